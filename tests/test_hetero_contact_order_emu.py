"""The key-ordered export and the matching report over the world groups of a heterogeneous model (nt_contacts_export_sorted_groups
/ _match_report_groups / _order_save_groups) on the emulated library, through the product's Python path: tests/
test_gpu_hetero_contact_order.py's order, empty-frame, per-group, matching, force and repeatability tests run unchanged on small
layouts.  (Its no-synchronisation and hipGraph tests stay with the device.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(TESTS, "emu"), ROOT, os.environ.get("PYTHONPATH", "")]))


def test_hetero_contact_order_and_matching_dry_run(oracle_lib):
    r = subprocess.run([sys.executable, "-m", "pytest", "-p", "emu_plugin", "-m", "gpu", "-q", "test_gpu_hetero_contact_order.py",
                        "-k", "not synchronise and not replays"], cwd=TESTS, env=ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "9 passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]

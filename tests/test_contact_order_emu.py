"""The key-ordered contact export and the matching report (include/newton_hip_contacts.h) on the emulated library, through the
product's Python path: tests/test_gpu_contact_order.py's order, empty-frame and report tests run unchanged on small scenes (slot
contacts of analytic and convex pairs, the SDF legs' rows, hydroelastic rows with their stiffness, a world reset and the broken list
after it) against a numpy stable sort of the default pipeline's raw export and against the report's definitions.  (Its hipGraph
tests stay with the device.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(TESTS, "emu"), ROOT, os.environ.get("PYTHONPATH", "")]))


def test_contact_order_and_report_dry_run(oracle_lib):
    r = subprocess.run([sys.executable, "-m", "pytest", "-p", "emu_plugin", "-m", "gpu", "-q", "test_gpu_contact_order.py",
                        "-k", "stable_sort or empty_frame or world_reset"], cwd=TESTS, env=ENV, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "8 passed" in r.stdout and "failed" not in r.stdout


def test_existing_matching_tests_take_the_device_path_dry_run(oracle_lib):
    """The pipeline-level matching tests (latest + report against oracle_match, sticky against the recorded reference vectors, the
    SDF rows' matching) and the standalone ContactMatcher on key-ordered contacts, unchanged, on the emulated library."""
    for f, k, want in (("test_zx_round2_gpu.py", "matching or matcher", "4 passed"), ("test_gpu_sdf_pipeline.py", "matching", "3 passed")):
        r = subprocess.run([sys.executable, "-m", "pytest", "-p", "emu_plugin", "-m", "gpu", "-q", f, "-k", k], cwd=TESTS, env=ENV,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert want in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]

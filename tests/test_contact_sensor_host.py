"""newton_amd.sensors.SensorContact on a host model: closed-form cases of the float64 path (contact_sensor_numpy, the reference of
contact_sensor_kernel), the constructor's errors, and the synthetic sets of tests/contact_sensor_cases.py against themselves (the order
set must not be vacuous: its float32 sequential sum differs from the float64, reversed and pairwise sums)."""
from types import SimpleNamespace

import numpy as np
import pytest

import contact_sensor_cases as cs
from newton_amd import sensors

E = 3


@pytest.fixture(scope="module")
def model():
    return cs.sensor_model(E)


def _contacts(model, entries):
    """entries: (world, slot0, slot1, force[3]) in flat order, followed by two entries beyond the count."""
    t = model.env
    s0 = [cs.shape_id(t, w, a) if a >= 0 else -1 for w, a, b, f in entries] + [cs.shape_id(t, 0, 0), -1]
    s1 = [cs.shape_id(t, w, b) if b >= 0 else -1 for w, a, b, f in entries] + [cs.shape_id(t, 0, t.ns), -1]
    force = np.zeros((len(s0), 6))
    for i, (w, a, b, f) in enumerate(entries):
        force[i, :3], force[i, 3:] = f, 9.0  # (the torque part is not read)
    force[len(entries)] = 100.0  # beyond the count: not read
    return SimpleNamespace(rigid_contact_count=np.array([len(entries)], np.int32), rigid_contact_shape0=np.array(s0, np.int32),
                           rigid_contact_shape1=np.array(s1, np.int32), force=force)


def test_sign_of_either_side_and_both_sides_sensing(model):
    t = model.env
    ground = t.ns
    s = sensors.SensorContact(model, sensing_shapes=[3, 5], counterpart_shapes=[ground, 5])
    assert s.shape == (2, 3) and s.sensing_labels == [("shape", 3), ("shape", 5)] and s.counterpart_labels == [("shape", ground), ("shape", 5)]
    f1, f2, f3 = np.array([1.0, 2.0, 3.0]), np.array([0.5, 0.0, -4.0]), np.array([10.0, 20.0, 30.0])
    s.eval(_contacts(model, [(1, 3, ground, f1),     # sensing shape on side 0: +f
                             (1, ground, 3, f2),     # on side 1: -f
                             (1, 3, 5, f3)]))        # both sides sensing: +f on shape 3 (counterpart: shape 5), -f on shape 5
    want = np.zeros((E, 2, 3, 3))
    want[1, 0, 0], want[1, 0, 1], want[1, 0, 2] = f1 - f2 + f3, f1 - f2, f3
    want[1, 1, 0] = -f3  # shape 3 is no counterpart: the total column only
    assert np.array_equal(s.net_force, want)


def test_body_is_the_union_of_its_shapes_and_a_global_counterpart(model):
    t = model.env
    shapes_of_body0 = np.flatnonzero(np.asarray(t.shape_body)[:t.ns] == 0)
    assert len(shapes_of_body0) == 2
    a, b = (int(x) for x in shapes_of_body0)
    ground, ball = t.ns, t.ns + 1
    s = sensors.SensorContact(model, sensing_bodies=[0], counterpart_shapes=[ball, ground], counterpart_bodies=[4])
    assert s.counterpart_labels == [("body", 4), ("shape", ball), ("shape", ground)] and s.shape == (1, 4)
    other = int(np.flatnonzero(np.asarray(t.shape_body)[:t.ns] == 4)[0])
    f = [np.array([1.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0]), np.array([0.0, 0.0, 4.0]), np.array([8.0, 8.0, 8.0]), np.array([5.0, 5.0, 5.0])]
    s.eval(_contacts(model, [(2, a, ground, f[0]), (2, b, ground, f[1]), (2, ball, b, f[2]), (2, a, other, f[3]),
                             (2, a, b, f[4]),        # both shapes in the same sensing object: +f, then -f
                             (2, a, 7, f[0]),        # no listed counterpart: the total only
                             (2, -1, -1, f[3]),      # inert
                             (0, 9, ground, f[3])]))  # no sensing shape
    want = np.zeros((E, 1, 4, 3))
    want[2, 0, 0] = f[0] + f[1] - f[2] + f[3] + f[0]
    want[2, 0, 1], want[2, 0, 2], want[2, 0, 3] = f[3], -f[2], f[0] + f[1]
    assert np.array_equal(s.net_force, want)


def test_include_total_off_and_world_mask(model):
    t = model.env
    ground = t.ns
    s = sensors.SensorContact(model, sensing_shapes=[2], counterpart_shapes=[ground], include_total=False)
    assert s.shape == (1, 1)
    f = np.array([1.0, 2.0, 3.0])
    contacts = _contacts(model, [(w, 2, ground, f * (w + 1)) for w in range(E)] + [(0, 2, 8, f)])
    s.net_force[...] = 7.0
    s.eval(contacts, world_mask=[True, False, True])
    assert np.array_equal(s.net_force[:, 0, 0], [f, [7.0] * 3, 3 * f])
    with pytest.raises(ValueError, match="world_mask"):
        s.eval(contacts, world_mask=[True])


def test_constructor_errors(model):
    t = model.env
    n = t.ns + t.ng
    with pytest.raises(ValueError, match="no sensing object"):
        sensors.SensorContact(model, counterpart_shapes=[0])
    with pytest.raises(ValueError, match=f"sensing body {t.nb} is out of range"):
        sensors.SensorContact(model, sensing_bodies=[t.nb])
    with pytest.raises(ValueError, match="sensing shape -1 is out of range"):
        sensors.SensorContact(model, sensing_shapes=[-1])
    with pytest.raises(ValueError, match=f"counterpart shape {n} is out of range"):
        sensors.SensorContact(model, sensing_shapes=[0], counterpart_shapes=[n])
    with pytest.raises(ValueError, match="counterpart body -1 is out of range"):
        sensors.SensorContact(model, sensing_shapes=[0], counterpart_bodies=[-1])
    with pytest.raises(ValueError, match="shape slot 1 is claimed by two sensing objects"):
        sensors.SensorContact(model, sensing_bodies=[0], sensing_shapes=[1])  # (body 0 carries slots 0 and 1)
    with pytest.raises(ValueError, match="shape slot 4 is claimed by two counterpart objects"):
        sensors.SensorContact(model, sensing_shapes=[0], counterpart_shapes=[4, 4])
    with pytest.raises(ValueError, match="no output column"):
        sensors.SensorContact(model, sensing_shapes=[0], include_total=False)
    sensors.SensorContact(model, sensing_shapes=[4], counterpart_shapes=[4])  # a slot may be both
    with pytest.raises(NotImplementedError, match="SensorContact: heterogeneous models are unsupported"):
        sensors.SensorContact(SimpleNamespace(is_heterogeneous=True), sensing_shapes=[0])


def test_launch_constants_are_the_kernels():
    assert cs.kernel_constants() == (cs.CS_THREADS, cs.CS_MAX_WPB, cs.CS_ITEMS)
    assert [cs.launch_shape(S * (int(tot) + C))[0] for S, C, tot in cs.SHAPES.values()] == [16, 8, 4, 2, 1, 1]
    assert cs.launch_shape(289)[1] < 289  # more cells than lanes


def test_exact_set_is_exact_and_order_set_is_not_vacuous():
    model = cs.sensor_model(5)
    case = cs.exact_case(model, 40, *cs.SHAPES["cells20"], rows="ragged", seed=1)
    cs.check_exact(case, case.reference().astype(np.float32))
    case = cs.order_case(model, 100, *cs.SHAPES["cells20"], rows="ragged", seed=2)
    seq = cs.order_alternatives(case)[0]
    cs.check_order(case, seq)
    assert np.any(case.rshape0 >= 0) and np.any(case.shape0 >= 0)  # spread over slots and rows

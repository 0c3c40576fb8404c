"""The head stabilizer without a GPU: the specification's exact ``fmaf`` against libm, what the parity inputs of
``tests/test_stabilizer_gpu.py`` cover (on the specification alone), the params mirror, ``HeadStabilizer.fit`` and
``ideal_targets``, and the tripod CPG over a dof list with neck dofs in it."""
import ctypes
import ctypes.util
import hashlib

import numpy as np
import pytest

import stabilizer_spec as spec

from flygym_amd import _native
from flygym_amd.controllers import NECK_DOFS, HeadStabilizer, TripodCPG, _StabilizerParams

F32 = np.float32


def _libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    return lambda a, b, c: np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)


def _midpoint_triples():
    """a b + c whose float64 sum is rounded ONTO a float32 rounding midpoint that the exact sum lies just beside: with
    a = 2^-12 (1 + 2^-k), b = -2^-12 (1 - 2^-k) the product is -2^-24 (1 - 2^-2k), so c + a b = (1 + 2^-23) - 2^-24 + 2^-(24 + 2k):
    just above the midpoint 1 + 2^-24 of 1 and 1 + 2^-23, and for k >= 15 the last term is below float64's last bit there.  Rounding
    the float64 sum to float32 breaks the tie to even (1), the fused operation rounds up (1 + 2^-23).  Scaled by powers of two, with
    both signs."""
    out = []
    for k in range(15, 24):
        for e in (-20, -3, 0, 5, 40):
            for sign in (1.0, -1.0):
                a = F32(2.0 ** -12 * (1 + 2.0 ** -k) * 2.0 ** e)
                b = F32(-(2.0 ** -12) * (1 - 2.0 ** -k))
                c = F32((1 + 2.0 ** -23) * 2.0 ** e)
                out.append((sign * a, b, sign * c))
    return tuple(np.array(v, dtype=F32) for v in zip(*out))


def test_the_emulated_fmaf_is_libms():
    """Bit patterns of the emulated fused multiply-add against libm's ``fmaf`` on random triples across exponents (among them
    addends that nearly cancel the product) and on the crafted midpoint triples; the naive ``float32(float64(a) b + c)`` differs
    from ``fmaf`` on the crafted ones — a condition on these inputs, not on any code under test."""
    fma = _libm_fmaf()
    rng = np.random.default_rng(5)
    n = 20000
    a = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-40, 40, n) * rng.choice([-1, 1], n)).astype(F32)
    b = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-40, 40, n) * rng.choice([-1, 1], n)).astype(F32)
    c = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-80, 80, n) * rng.choice([-1, 1], n)).astype(F32)
    near = rng.random(n) < 0.4                                                      # addends of the product's size, often cancelling
    c[near] = (-(a[near].astype(np.float64) * b[near]) * (1 + rng.normal(0, 1, int(near.sum())) * 2.0 ** -rng.integers(1, 30, int(near.sum())))).astype(F32)
    c[::97] = 0
    a[::101] = 0
    assert spec.fmaf(a, b, c).view(np.uint32).tolist() == fma(a, b, c).view(np.uint32).tolist()
    ma, mb, mc = _midpoint_triples()
    want = fma(ma, mb, mc)
    assert spec.fmaf(ma, mb, mc).view(np.uint32).tolist() == want.view(np.uint32).tolist()
    naive = (ma.astype(np.float64) * mb.astype(np.float64) + mc.astype(np.float64)).astype(F32)
    wrong = int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"naive double rounding differs from fmaf on {wrong} of {len(ma)} crafted triples")
    assert wrong >= 1


@pytest.mark.parametrize("name", spec.ARCHITECTURES)
def test_the_parity_inputs_cover_the_network(name):
    """On the specification alone, over the population the GPU tests draw from: every hidden unit is active somewhere and clipped
    somewhere, every leg's flag takes both values, a leg touches with a force below its threshold, every output is clamped at
    ``lo``, clamped at ``hi`` and left strictly in between, and every intermediate — inputs, squared forces, every partial sum of
    every chain — is zero or a normal float32 (so flushing of denormals could not show)."""
    net = spec.network(name)
    lo, hi = spec.bounds(name)
    y, trace = spec.reference_run(name, spec.N_TOTAL)
    assert y.shape == (spec.UPDATES, spec.N_TOTAL, net.n_out) and y.dtype == F32
    assert [W.shape for W, _ in net.layers] == [(b, a) for a, b in zip([net.n_in, *spec.ARCHITECTURES[name][2]], [*spec.ARCHITECTURES[name][2], net.n_out])]
    for i, a in enumerate(trace["hidden"]):
        flat = a.reshape(-1, a.shape[-1])
        assert (flat > 0).any(axis=0).all() and (flat <= 0).any(axis=0).all(), (name, "hidden layer", i)
    if net.contacts:
        flags = trace["flags"].reshape(-1, 6)
        assert flags.any(axis=0).all() and (~flags).any(axis=0).all()
        assert trace["found_below"].reshape(-1, 6).any(axis=0).all()
    u = trace["unclamped"].reshape(-1, net.n_out)
    assert (lo < hi).all()
    assert (u < lo).any(axis=0).all() and (u > hi).any(axis=0).all() and ((u > lo) & (u < hi)).any(axis=0).all()
    flat = y.reshape(-1, net.n_out)
    assert (flat == lo).any(axis=0).all() and (flat == hi).any(axis=0).all() and (flat >= lo).all() and (flat <= hi).all()
    tiny = float(np.finfo(F32).tiny)
    assert trace["smallest_nonzero"] >= tiny and np.isfinite(trace["largest"]) and trace["largest"] < 1e6, (trace["smallest_nonzero"], trace["largest"])
    # a smaller batch holds the population's last worlds
    for n in spec.WORLDS[:-1]:
        assert spec.reference_run(name, n)[0].tobytes() == np.ascontiguousarray(y[:, spec.N_TOTAL - n:]).tobytes()


def test_params_struct_matches_the_library():
    """The library loads without a GPU; the ctypes mirror has the layout it was compiled with."""
    _native.build()
    L = _native.lib()
    assert ctypes.sizeof(_StabilizerParams) == L.nmf_stabilizer_params_size() == 116
    for name in ("nmf_stabilizer_params_size", "nmf_stabilizer_create", "nmf_stabilizer_destroy", "nmf_stabilizer_update",
                 "nmf_stabilizer_field_ptr"):
        assert name in _native.exported_symbols() and hasattr(L, name)


def test_fit_is_deterministic_and_learns_a_teacher():
    """Data from a random teacher network (10 joint angles with offsets and scales, 6 flags): two runs with one seed give
    byte-identical arrays of the right shapes, another seed does not, the joint columns alone are standardised, and the fitted
    network's loss is below that of predicting the targets' mean."""
    rng = np.random.default_rng(3)
    n, n_q = 600, 10
    joints = rng.normal(0, 1, (n, n_q)) * rng.uniform(0.2, 2.0, n_q) + rng.normal(0, 1, n_q)
    flags = (rng.random((n, 6)) < 0.5).astype(np.float64)
    X = np.concatenate([joints, flags], axis=1).astype(F32)
    teacher = [(rng.normal(0, 0.5, (12, 16)), rng.normal(0, 0.2, 12)), (rng.normal(0, 0.5, (2, 12)), rng.normal(0, 0.2, 2))]
    Z = np.concatenate([(joints - joints.mean(0)) / joints.std(0), flags], axis=1)
    Y = spec.relu_mlp(teacher, Z).astype(F32)
    runs = [HeadStabilizer.fit(X, Y, epochs=150, seed=4) for _ in range(2)]
    (layers, mean, std), (layers2, mean2, std2) = runs
    assert [(W.shape, b.shape) for W, b in layers] == [((32, 16), (32,)), ((32, 32), (32,)), ((2, 32), (2,))]
    assert all(a.dtype == F32 for W, b in layers for a in (W, b)) and mean.dtype == std.dtype == F32 and mean.shape == std.shape == (n_q,)
    for (W, b), (W2, b2) in zip(layers, layers2):
        assert W.tobytes() == W2.tobytes() and b.tobytes() == b2.tobytes()
    assert mean.tobytes() == mean2.tobytes() and std.tobytes() == std2.tobytes()
    other, _, _ = HeadStabilizer.fit(X, Y, epochs=5, seed=5)
    again, _, _ = HeadStabilizer.fit(X, Y, epochs=5, seed=4)
    assert other[0][0].tobytes() != again[0][0].tobytes()
    np.testing.assert_allclose(mean, joints.mean(0), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(std, joints.std(0, ddof=1), rtol=1e-4)
    small, _, _ = HeadStabilizer.fit(X, Y, hidden=(5,), epochs=3)
    assert [W.shape for W, _ in small] == [(5, 16), (2, 5)]
    fitted = spec.relu_mlp(layers, np.concatenate([(X[:, :n_q] - mean) / std, X[:, n_q:]], axis=1))
    final, baseline = float(((fitted - Y) ** 2).mean()), float(((Y.mean(0) - Y) ** 2).mean())
    print(f"fit: loss {final:.4g} against {baseline:.4g} for the targets' mean")
    assert final < baseline
    with pytest.raises(ValueError, match="inputs"):
        HeadStabilizer.fit(X, Y[:-1])


def test_ideal_targets_against_float64():
    """Minus the thorax's roll and pitch against a float64 evaluation of the same float32 quaternions, at attitudes with
    |pitch| <= 60 degrees, ``atol=1e-5`` rad: float32 ``asin`` / ``atan2`` are good to a few ulp of their arguments and results
    (about 1e-7 relative), the angles' conditioning is at most 1 / cos(60 deg) = 2 there, which gives about 1e-6 on angles up to
    pi; the tolerance is a factor 10 over that."""
    import torch

    rng = np.random.default_rng(8)
    n = 4000
    roll, yaw = rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n)
    pitch = rng.uniform(-np.pi / 3, np.pi / 3, n)
    roll[:3], pitch[:3], yaw[:3] = (0.0, 0.5, -0.5), (0.0, -np.pi / 3, np.pi / 3), (0.0, 1.0, 2.0)
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    quat = np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=1)
    q32 = quat.astype(F32)
    got = HeadStabilizer.ideal_targets(torch.as_tensor(q32).reshape(40, 100, 4))
    assert tuple(got.shape) == (40, 100, 2) and got.dtype == torch.float32
    w, x, y, z = q32.astype(np.float64).T
    want = np.stack([-np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), -np.arcsin(np.clip(2 * (w * y - z * x), -1, 1))], axis=1)
    err = np.abs(got.reshape(-1, 2).numpy().astype(np.float64) - want)
    print(f"ideal_targets: largest error {err.max():.3g} rad")
    assert err.max() <= 1e-5
    # and they are the angles the quaternions were built from
    wrap = lambda a: (a + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(wrap(want[:, 0] + roll)).max() < 1e-5 and np.abs(want[:, 1] + pitch).max() < 1e-5
    assert got[0, 0].tolist() == [0.0, 0.0]


# sha256 of TripodCPG(make_model()'s 42 leg dofs, 1e-4).cycle as the parent of this feature computed it
CYCLE_SHA256 = "09964d56d4605ac71b3bab6b16330bce75ee70cd8397d649afe896313464fcd4"


def test_the_tripod_cpg_takes_the_leg_dofs_of_a_list_with_neck_dofs():
    """Over a dof list with the neck's roll and pitch mixed in, the CPG keeps the leg dofs as its columns and builds the same step
    cycle; without them its cycle has the bytes it had before the CPGs learned to skip other dofs."""
    from flygym_amd import make_model
    from flygym_amd.anatomy import JointDOF

    fly, _, _ = make_model()
    legs = fly.get_actuated_jointdofs_order("position")
    neck = [JointDOF.from_name(name) for name in NECK_DOFS]
    plain = TripodCPG(legs, 1e-4)
    assert plain.actuated_dofs == legs and plain.leg_columns.tolist() == list(range(42)) and plain.cycle.shape == (256, 42)
    assert hashlib.sha256(plain.cycle.tobytes()).hexdigest() == CYCLE_SHA256
    mixed = TripodCPG([neck[0], *legs[:10], neck[1], *legs[10:]], 1e-4)
    assert mixed.actuated_dofs == legs and mixed.leg_columns.tolist() == [*range(1, 11), *range(12, 44)]
    assert mixed.cycle.tobytes() == plain.cycle.tobytes() and np.array_equal(mixed.leg_of_dof, plain.leg_of_dof)
    assert mixed.targets(2, 3).tobytes() == plain.targets(2, 3).tobytes()

"""The visual-network specification (``tests/visnet_spec.py``) against what it promises, ``Retina.hex_neighbours`` and the
build-defined default network ``sensors.motion_pathway`` — no GPU.

Drifting sine gratings on the default retina in the protocol of ``tests/test_motion_cpu.py``: wavelength six lattice pitches,
contrast 0.4 about 0.5, ``dt`` = 2 ms, 2 Hz, the pooled responses averaged over the second half of 500 ticks (one whole period).
Run once for all stimuli (one world each, a stimulus per eye), shared and read-only."""
import ctypes
import functools

import numpy as np
import pytest

import visnet_spec as spec

f32 = np.float32
PARITY = [("smallest", 1), ("ring", 2), ("ragged", 1), ("ragged", 3), ("widest", 1), ("square", 1)]
TICKS = 500
DRIFT = {"+x": (1.0, 0.0), "-x": (-1.0, 0.0), "+y": (0.0, 1.0), "-y": (0.0, -1.0), "still": None}
# a stimulus per eye (left, right), in lattice coordinates: the same table serves both eyes here, so +x is front to back
WORLDS = [("+x", "-x"), ("-x", "+x"), ("+y", "-y"), ("+x", "+x"), ("still", "still")]
PREFERRED = {"ftb": "+x", "btf": "-x", "down": "+y", "up": "-y"}


def test_the_default_retinas_lattice():
    r = spec.retina("default")
    table, offsets = r.hex_neighbours()
    assert table.shape == (19, 721) and table.dtype == np.int32 and offsets.shape == (19, 2) and offsets.dtype == np.float64
    valid = table >= 0
    assert valid.sum(axis=1).tolist() == [721] + [690] * 6 + [660] * 6 + [659] * 6
    assert int(valid.sum()) == 12775 and int(valid.all(axis=0).sum()) == 547
    assert np.array_equal(table[0], np.arange(721)) and not offsets[0].any()
    pitch = np.hypot(offsets[1:7, 0], offsets[1:7, 1]).mean()
    length = np.hypot(offsets[:, 0], offsets[:, 1]) / pitch
    assert np.abs(length[1:7] - 1).max() < 0.01 and np.abs(length[7:13] - np.sqrt(3)).max() < 0.02 and np.abs(length[13:] - 2).max() < 0.02
    angle = np.arctan2(offsets[:, 1], offsets[:, 0])
    for ring in (slice(1, 7), slice(7, 13), slice(13, 19)):
        assert (np.diff(angle[ring]) > 0).all()                                        # ascending atan2 inside a class
    c = r.ommatidia_centres()
    worst = max(np.hypot(*(c[valid[t]] + offsets[t] - c[table[t, valid[t]]]).T).max() for t in range(19)) / pitch
    print(f"default retina: pitch {pitch:.3f} pixels, worst matched error {worst:.4f} pitch")
    assert worst < 0.05                                                                 # (a fifth of the matching radius)
    for t in range(1, 19):                                                              # tap t and its opposite undo each other
        back = int(np.argmin(np.hypot(*(offsets + offsets[t]).T)))
        assert np.hypot(*(offsets[back] + offsets[t])) < 0.02 * pitch and back != t
        there = table[t]
        both = (there >= 0) & (table[back, np.maximum(there, 0)] >= 0)
        assert both.sum() == valid[t].sum() and np.array_equal(table[back, there[both]], np.nonzero(both)[0])
    for rings, T in ((0, 1), (1, 7)):
        few, off = r.hex_neighbours(rings)
        assert np.array_equal(few, table[:T]) and np.array_equal(off, offsets[:T])
    with pytest.raises(ValueError, match="rings"):
        r.hex_neighbours(3)


def test_small_retinas_and_retinas_without_a_hexagonal_lattice():
    from flygym_amd.sensors import Retina, eye_tables

    seven = spec.retina("seven")
    assert seven.num_ommatidia == 7
    table, offsets = seven.hex_neighbours(2)
    assert table.shape == (19, 7) and np.array_equal(table[0], np.arange(7))
    centre = int(np.argmin(np.hypot(*(seven.ommatidia_centres() - seven.ommatidia_centres().mean(axis=0)).T)))
    assert (table[1:7, centre] >= 0).all() and sorted(table[1:7, centre].tolist()) == [i for i in range(7) if i != centre]
    assert (table[7:, centre] == -1).all() and (table[1:7] >= 0).sum() == 6 + 6 * 3     # a rim cell: the centre and two rim cells
    assert (table[7:13] >= 0).sum() == 6 * 2 and (table[13:] >= 0).sum() == 6            # across the rim: sqrt(3) twice, 2 once
    one = spec.retina("one")
    table, offsets = one.hex_neighbours(0)
    assert table.tolist() == [[0]] and offsets.tolist() == [[0.0, 0.0]]
    with pytest.raises(ValueError, match="at least 7"):
        one.hex_neighbours(1)
    with pytest.raises(ValueError, match="not a hexagonal lattice"):
        spec.retina("square").hex_neighbours()
    with pytest.raises(ValueError, match="1024"):
        Retina(id_map=np.arange(1, 1026, dtype=np.int16).reshape(25, 41)).hex_neighbours()
    # per eye: the eye whose last column faces forward reads its taps mirrored in x
    both, offsets = eye_tables(spec.retina("default"), front_edge=(1, 0))
    plain = spec.retina("default").hex_neighbours()[0]
    assert both.shape == (2, 19, 721) and np.array_equal(both[1], plain)
    for t in range(19):
        mirror = int(np.argmin(np.hypot(*(offsets * [-1, 1] - offsets[t]).T)))
        assert np.array_equal(both[0, t], plain[mirror])
    assert np.array_equal(eye_tables(spec.retina("default"), front_edge=(0, 0))[0][0], plain)


@functools.lru_cache(maxsize=None)
def _parity(name, substeps):
    """The parity protocol of ``spec.run`` with the float64 twin beside it: per update ``(v32, out32, v64, bound, pooled64)``."""
    flat, table, which = spec.case(name, substeps)
    n_omm = spec.retina(which).num_ommatidia
    omm, base = spec.readings(n_omm), spec.bases()
    s32 = spec.new_state(spec.N_TOTAL, flat.n_types, n_omm)
    s64 = spec.new_state(spec.N_TOTAL, flat.n_types, n_omm, np.float64)
    out = []
    for k in range(spec.UPDATES):
        got = spec.update(s32, omm[k], flat, table, **{**spec.PARAMS, "base": base if k % 2 else spec.PARAMS["base"]})
        twin = spec.update64(s64, omm[k], flat, table)
        out.append((s32["v"].copy(), got, s64["v"].copy(), twin["bound"], twin["pooled"]))
    return out


def test_the_parity_runs_are_the_ones_of_the_gpu_tests():
    for name, substeps in (("ring", 2), ("ragged", 3)):
        flat, table, which = spec.case(name, substeps)
        for mine, (state, theirs) in zip(_parity(name, substeps), spec.run(flat, table, spec.retina(which).num_ommatidia, spec.N_TOTAL)):
            assert np.array_equal(mine[0].view(np.int32), state["v"].view(np.int32)) and np.array_equal(mine[1]["drive"], theirs["drive"])


@pytest.mark.parametrize("name,substeps", PARITY)
def test_what_the_parity_inputs_cover(name, substeps):
    """On the specification alone: every type is active in some cell and silent in another; the pooling clamp; missing
    neighbours; the drive on both clamps and between them; nothing that is not finite."""
    runs = _parity(name, substeps)
    flat, table, _ = spec.case(name, substeps)
    r_min = np.min([out["r_min"] for _, out, *_ in runs], axis=0)
    r_max = np.max([out["r_max"] for _, out, *_ in runs], axis=0)
    assert (r_min == 0).all() and (r_max > 0).all(), (r_min, r_max)
    assert all(out["finite"] for _, out, *_ in runs)
    clamped = sum(out["clamped"] for _, out, *_ in runs)
    missing = sum(out["missing"] for _, out, *_ in runs)
    drive = np.stack([out["drive"] for _, out, *_ in runs])
    lo, hi = f32(spec.DEFAULTS["drive_min"]), f32(spec.DEFAULTS["drive_max"])
    assert (drive == lo).any() and ((drive > lo) & (drive < hi)).any()                  # (every case: world 0's left base is 0.1)
    print(f"{name}, substeps {substeps}: {clamped} cells on the pooling clamp, {missing} taps on a missing neighbour, "
          f"drive {float(drive.min()):.3f} .. {float(drive.max()):.3f}")
    if name in ("smallest", "ring"):
        assert clamped == 0                                                             # (the clamp is missed here, hit below)
    else:
        assert clamped > 0
    assert (missing == 0) == (name == "smallest")
    if name != "ragged":
        assert (drive == hi).any()
    if name == "square":
        assert (np.asarray(table) == -1).any() and np.asarray(table).shape == (2, 19, 1024)


@pytest.mark.parametrize("name,substeps", PARITY)
def test_the_float32_rule_stays_within_its_bound_of_the_float64_twin(name, substeps):
    """``update64`` carries the bound, derived in its docstring from the rule's own roundings; the pooled responses add half a unit
    of the 2^-16 grid and the final rounding to float32."""
    for k, (v32, out, v64, bound, pooled64) in enumerate(_parity(name, substeps)):
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        perr = float(np.abs(out["pooled"].astype(np.float64) - pooled64).max())
        print(f"{name}, substeps {substeps}, update {k}: |v32 - v64| <= {err:.3e} (bound {bound:.3e}), pooled {perr:.3e}")
        assert err <= bound
        assert perr <= bound + 2.0 ** -17 + spec.CLAMP * spec.U


@functools.lru_cache(maxsize=None)
def _gratings():
    """``dict(pooled (worlds, 2, C), drive (worlds, 2), signal (worlds,): means over the second half; names)``."""
    from flygym_amd import sensors

    r = spec.retina("default")
    table, offsets = r.hex_neighbours(2)
    network = sensors.motion_pathway(offsets)
    names, types, edges, taps, tap_w = sensors.flatten_network(network, spec.DT)
    flat = spec.Flat(types, edges, taps, tap_w, np.array([network.tau[t] for t in names]), 1)
    c = r.ommatidia_centres()
    lam = 6.0 * np.hypot(*offsets[1])
    along = np.array([[c @ np.array(DRIFT[d] or (1.0, 0.0)) for d in world] for world in WORLDS])          # (worlds, 2, n_omm)
    freq = np.array([[0.0 if DRIFT[d] is None else 2.0 for d in world] for world in WORLDS])[:, :, None]
    pale = r.pale_mask != 0
    n = len(WORLDS)
    state = spec.new_state(n, len(names), 721)
    acc = dict(pooled=np.zeros((n, 2, len(names))), drive=np.zeros((n, 2)), signal=np.zeros(n))
    for k in range(TICKS):
        x = (0.5 + 0.4 * np.sin(2.0 * np.pi * (along / lam - freq * (k * spec.DT)))).astype(f32)
        omm = np.stack([np.where(pale, 0, x), np.where(pale, x, 0)], axis=-1).astype(f32)
        out = spec.update(state, omm, flat, table, gain=10.0)
        assert out["finite"]
        if k >= TICKS // 2:
            for key in acc:
                acc[key] += out[key]
    return {**{key: value / (TICKS - TICKS // 2) for key, value in acc.items()}, "names": names}


SEEN_BY = {"+x": (0, 0), "-x": (0, 1), "+y": (2, 0), "-y": (2, 1), "still": (4, 0)}          # drift -> (world, eye) of WORLDS


def _response(kind, drift):
    g = _gratings()
    world, eye = SEEN_BY[drift]
    assert WORLDS[world][eye] == drift
    return float(g["pooled"][world, eye, g["names"].index(kind)])


def test_every_directional_type_prefers_its_own_direction():
    """Measured with this specification (pooled response, preferred : opposite : across : still): T4 0.195 : 0.139 : 0.104 : 0.007
    along x and 0.181 : 0.126 : 0.103 : 0.001 along y; T5 0.167 : 0.118 : 0.087 : 0 and 0.155 : 0.107 : 0.087 : 0."""
    for cell in ("T4", "T5"):
        for name, own in PREFERRED.items():
            kind = cell + name
            resp = {d: _response(kind, d) for d in DRIFT}
            others = [resp[d] for d in PREFERRED.values() if d != own]
            print(f"{kind}: preferred {resp[own]:.4f}, others {[round(v, 4) for v in others]}, still {resp['still']:.4f}; "
                  f"preferred : opposite = {resp[own] / max(others):.2f}")
            assert resp[own] > max(others) and resp["still"] < resp[own], (kind, resp)


def test_the_signal_measures_rotation_and_ignores_translation():
    """Front to back across the left eye and back to front across the right one — the panorama turning counter-clockwise — slows
    the left side; the mirrored stimulus the right side; the same grating on both eyes neither."""
    g = _gratings()
    print(f"signal {g['signal'].round(4).tolist()}, drive {g['drive'].round(4).tolist()}")
    assert g["signal"][0] > 0 and g["drive"][0, 0] < g["drive"][0, 1]
    assert g["signal"][1] < 0 and g["drive"][1, 1] < g["drive"][1, 0]
    assert g["signal"][3] == 0 and g["drive"][3, 0] == g["drive"][3, 1]
    assert g["drive"][4, 0] == g["drive"][4, 1]


def test_networks_by_name_flatten_to_the_arrays_of_the_abi():
    from flygym_amd import sensors

    net = sensors.motion_pathway(spec.retina("default").hex_neighbours(1)[1])
    names, types, edges, taps, tap_w = sensors.flatten_network(net, 0.002, 2)
    assert len(names) == 15 and names[:7] == ("Lm", "On", "Off", "OnF", "OnD", "OffF", "OffD") and types.shape == (15, 5)
    assert types.dtype == f32 and edges.dtype == taps.dtype == np.int32 and tap_w.dtype == f32 and len(taps) == len(tap_w) == 54
    assert np.array_equal(types[:, 3], spec.coefficient(0.002, [net.tau[t] for t in names], 2))
    assert edges[0].tolist() == [1, 0] and taps[0].tolist() == [0, 0] and tap_w[0] == -1
    again = sensors.flatten_network(dict(types=net.types, tau=net.tau, bias=net.bias, in_w=net.in_w, steer_w=net.steer_w, edges=net.edges), 0.002, 2)
    assert all(np.array_equal(a, b) for a, b in zip(again[1:], (types, edges, taps, tap_w)))
    flat = sensors.FlatNetwork(names, [net.tau[t] for t in names], types[:, 0], types[:, 1:3], types[:, 4], edges, taps, tap_w)
    assert all(np.array_equal(a, b) for a, b in zip(sensors.flatten_network(flat, 0.002, 2)[1:], (types, edges, taps, tap_w)))
    steer = dict(zip(names, types[:, 4].tolist()))
    assert steer["T4ftb"] == steer["T5ftb"] == 1 and steer["T4btf"] == steer["T5btf"] == -1 and sum(map(abs, steer.values())) == 4


def test_the_params_mirror_has_the_librarys_size():
    from flygym_amd import _native
    from flygym_amd.sensors import _VisnetParams

    assert ctypes.sizeof(_VisnetParams) == _native.lib().nmf_visnet_params_size() == 44

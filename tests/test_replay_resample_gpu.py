"""``nmf_replay_resample_kernel`` (csrc/nmf_replay.hip) against its own restatement, oracle/replay_oracle.py, on every case
of tests/test_replay_oracle_cpu.py — where that module holds the oracle to the scipy pipeline — and the ABI's refusals.

The calls go through ``_native.lib()`` as ``MotionSnippet.get_joint_angles_device`` makes them.  Every case runs twice: with
the reference's row count ``len(arange(0, n / fps, dt))`` and with 300 rows more, which the ABI allows and which holds the last
smoothed frame far past the last knot.

The oracle is the kernel's arithmetic in numpy float64; the compiler may contract the kernel's float64 expressions into FMAs,
reorder its sums and turn its divisions by ``fps`` into products, so a float64 value can differ by about 1e-16 and, rarely,
round to the other float32 — in the output, or in a smoothed frame (the exact smoothed value of float32 samples is an exact
float32 tie in 77 of the 107 380 frames of the 1536 x 70 case, and the last bit of the float64 sum decides it), which then
moves the outputs around that frame by up to one ulp of the frame.  The bar, as tests/test_replay_oracle_cpu.py and the
shipped clip's test (tests/test_hip_parity_r2.py) have it: no value further off than one float32 ulp of its column's largest
smoothed magnitude; every call of fewer than 1000 values bit-identical; and, pooled over the whole table (3.5 million values),
at most 1e-3 of the values different in any bit.

Measured on an MI355X: 12 of 3 537 778 values differ (pooled share 3.4e-6), all in the 1536 x 70 case — the same 6 outputs
in each of its two calls; 19 of the 20 cases are bit-identical.  Four of the 6 are rows 550..558 of column 30, around frame
138: an exact tie, which summing sample by sample and numpy's dot product round differently on the host as well; the other two
are single outputs.  The worst is 0.125 ulp of its column's largest smoothed magnitude — and 2 ulp of its own, small, value:
an ulp taken of the value itself (as the first version of this test took it) is no measure for a float64 difference of 1e-16
relative to the frames."""

import ctypes

import numpy as np
import pytest

from test_replay_oracle_cpu import CASES, IDS, column_ulp, make_clip, n_out_of, oracle_table, smoothed

pytestmark = pytest.mark.gpu
EXTRA_ROWS = 300


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _resample(torch, clip, case, n_out):
    """One call of the ABI -> float32 (n_out, n_cols) numpy."""
    from flygym_amd import _native
    from flygym_amd.replay import savgol_taps

    n, window, polyorder, fps, dt, n_cols, _ = case
    clip_d = torch.as_tensor(np.ascontiguousarray(clip, dtype=np.float32), device="cuda:0")
    taps = torch.as_tensor(savgol_taps(window, polyorder), device="cuda:0")
    assert taps.dtype == torch.float64 and taps.numel() == window + 2 * (window // 2) * window
    out = torch.full((n_out, n_cols), float("nan"), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream(clip_d.device).cuda_stream
    _native.check(_native.lib().nmf_replay_resample(clip_d.data_ptr(), n, n_cols, float(fps), float(dt), taps.data_ptr(), window,
                                                    n_out, out.data_ptr(), stream))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def tables(torch_mod):
    """case -> (kernel table, kernel table with 300 rows more, oracle table with 300 rows more), computed once."""
    res = {}
    for case in CASES:
        clip, n_out = make_clip(case), n_out_of(case)
        res[case] = (_resample(torch_mod, clip, case, n_out), _resample(torch_mod, clip, case, n_out + EXTRA_ROWS),
                     oracle_table(case, clip, n_out + EXTRA_ROWS))
    return res


def _neq(a, b):
    return a.view(np.uint32) != b.view(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_its_oracle(tables, case):
    got, got_more, want_more = tables[case]
    n_out = n_out_of(case)
    want = want_more[:n_out]            # the oracle's default grid is the same rows (tests/test_replay_oracle_cpu.py)
    assert got.shape == (n_out, case[5]) and got_more.shape == want_more.shape == (n_out + EXTRA_ROWS, case[5])
    ulp = column_ulp(smoothed(case, make_clip(case)))[None, :]
    for name, g, w in (("reference grid", got, want), ("300 rows more", got_more, want_more)):
        assert np.isfinite(g).all(), f"{name}: rows the kernel did not write"
        neq = _neq(g, w)
        err = np.abs(g.astype(np.float64) - w.astype(np.float64))
        own = np.spacing(np.maximum(np.abs(g), np.abs(w))).astype(np.float64)
        print(f"{case} {name}: {int(neq.sum())} of {neq.size} values differ at (row, column) {np.argwhere(neq)[:12].tolist()}, worst "
              f"{float((err / ulp).max()):.3f} ulp of the column's largest smoothed magnitude, {float((err / own).max()):.3f} ulp of the value")
        assert (err <= ulp).all(), f"{name}: {int((err > ulp).sum())} values more than one float32 ulp off, worst {float((err / ulp).max()):.3g} ulp"
        if g.size < 1000:
            assert not neq.any(), f"{name}: {int(neq.sum())} of {g.size} values differ"
    # past the last knot every row is the last smoothed frame, bit for bit the same row
    np.testing.assert_array_equal(got_more[n_out:].view(np.uint32), np.broadcast_to(got_more[-1].view(np.uint32), (EXTRA_ROWS, case[5])))
    np.testing.assert_array_equal(got_more[:n_out].view(np.uint32), got.view(np.uint32))       # the row count changes no row


def test_pooled_share_of_differing_values(tables):
    """At most 1e-3 of all values of the table may differ from the oracle in any bit (an upper bound, not a fit).
    Measured on an MI355X: 12 of 3 537 778, a share of 3.4e-6."""
    neq = total = 0
    for case in CASES:
        got, got_more, want_more = tables[case]
        neq += int(_neq(got, want_more[:len(got)]).sum()) + int(_neq(got_more, want_more).sum())
        total += got.size + got_more.size
    print(f"pooled: {neq} of {total} values differ from the oracle: share {neq / total:.3e}")
    assert total > 300_000
    assert neq / total <= 1e-3, f"{neq} of {total} values differ"


def test_refusals_leave_the_output_untouched(torch_mod):
    """Every argument the ABI refuses: a nonzero return, ``nmf_last_error`` naming the call, nothing written."""
    torch = torch_mod
    from flygym_amd import _native
    from flygym_amd.replay import savgol_taps

    L = _native.lib()
    n, window, cols, n_out = 9, 5, 3, 40
    clip = torch.as_tensor(np.random.default_rng(0).uniform(-3, 3, (1537, cols)).astype(np.float32), device="cuda:0")
    # (clip and taps are large enough for every refused size, should one be accepted after all)
    taps = torch.as_tensor(np.concatenate([savgol_taps(window, 3), np.zeros(200)]), device="cuda:0")
    out = torch.full((n_out, cols), -77.0, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream(clip.device).cuda_stream
    good = dict(clip=clip.data_ptr(), n=n, cols=cols, fps=100.0, dt=0.0025, taps=taps.data_ptr(), window=window, n_out=n_out, out=out.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        return L.nmf_replay_resample(a["clip"], a["n"], a["cols"], a["fps"], a["dt"], a["taps"], a["window"], a["n_out"], a["out"], stream)

    bad = [(dict(n=5), b"n_frames"), (dict(n=1537), b"n_frames"), (dict(window=4), b"window"), (dict(window=1), b"window"),
           (dict(window=n + 2), b"window"), (dict(cols=0), b"sizes"), (dict(n_out=0), b"sizes"), (dict(fps=0.0), b"rates"),
           (dict(fps=float("nan")), b"rates"), (dict(dt=0.0), b"rates"), (dict(dt=float("nan")), b"rates"),
           (dict(clip=None), b"null"), (dict(taps=None), b"null"), (dict(out=None), b"null")]
    for kw, word in bad:
        rc = call(**kw)
        assert rc != 0, f"{kw} was accepted"
        msg = L.nmf_last_error()
        assert b"nmf_replay_resample" in msg and word in msg, (kw, msg)
        with pytest.raises(_native.NativeError):
            _native.check(rc)
        torch.cuda.synchronize()
        assert bool((out == -77.0).all()), f"{kw}: the refused call wrote to the output"
    # the process is still usable, and the good arguments are good
    out.fill_(-77.0)
    assert call() == 0
    torch.cuda.synchronize()
    want = oracle_table((n, window, 3, 100.0, 0.0025, cols, 0), clip[:n].cpu().numpy(), n_out)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))

"""The retina kernels of csrc/nmf_sensors.hip at the map sizes where their loops split.

``nmf_retina_kernel`` (any pixel count that is a multiple of 16) and ``nmf_retina_stream_kernel`` (multiples of 1024, with the
run plan of ``nmf_retina_plan_kernel`` / ``nmf_retina_active_kernel``) sum bytes in integers, so every reading here is compared
bit for bit with ``sensors_oracle.retina_resample``, through ``Retina(id_map=..., pale_mask=...).raw_image_to_hex_pxls``.
tests/test_sensors.py runs the default lattice, a 2-chunk map and a 2-group map; here:

* 1539 chunks on the non-streaming kernel: every thread takes one two-chunk iteration, threads 0..2 a second, the others the
  one-chunk loop; and once more from buffers that hold one chunk more than the kernel may read;
* 9, 16 and 17 groups on the streaming kernel: the two-group iteration with its second LDS stage, alone, before and without
  the one-group remainder, on images whose paired groups hold different bytes;
* a hand-built map of every run structure a 16-pixel chunk can have, on both kernels, and its plan words;
* 1024 ommatidia (the LDS accumulator's size), and the refusal of 1025;
* the refusal of a pixel count that is no multiple of 16.  The ABI demands ``3 * n_pixels % 16 == 0``, so the tail-pixel loop at
  the end of ``nmf_retina_kernel`` (``n_pix`` not a multiple of 16) cannot be reached through it: no test here tries to;
* the plan blob (per-chunk words, ascending list of the chunks that touch an ommatidium, their count) against a numpy
  restatement, with an active list that crosses wave and 256-chunk borders with empty and full waves."""

import numpy as np
import pytest

from flygym_amd.sensors import Retina

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch


def _check(torch, retina, imgs):
    """HIP readings of ``imgs`` (n, H, W, 3) == the numpy specification, every bit."""
    import sensors_oracle as so

    got = retina.raw_image_to_hex_pxls(torch.as_tensor(imgs, device="cuda:0")).cpu().numpy()
    want = so.retina_resample(imgs, retina.id_map, retina.pale_mask, retina.inv_norm)
    assert got.shape == want.shape == (len(imgs), retina.num_ommatidia, 2)
    assert want.max() > 0
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    return got


def _run_map(rng, shape, n_omm, run_length):
    """An id map of random runs (ids 0..n_omm, 0 = background; ``run_length(k)`` pixels for run k) in which every id occurs."""
    n_pix, ids, k = shape[0] * shape[1], [], 0
    while len(ids) < n_pix:
        ids += [int(rng.integers(0, n_omm + 1))] * run_length(k)
        k += 1
    ids = np.array(ids[:n_pix], dtype=np.int16)
    ids[:n_omm] = np.arange(1, n_omm + 1)
    return ids.reshape(shape)


def _hostile_runs(rng):
    """The run lengths of the 2-group map of tests/test_sensors.py: 1..9 pixels, every third run 8..29."""
    return lambda k: int(rng.integers(1, 10)) if k % 3 else int(rng.integers(8, 30))


def test_two_chunk_loop_of_the_plain_kernel(torch_mod):
    rng = np.random.default_rng(11)
    id_map = _run_map(rng, (27, 912), 60, lambda k: int(rng.integers(1, 41)))
    assert id_map.size == 16 * 1539 and id_map.size % 1024 != 0 and (id_map == 0).mean() > 0.005
    pale = rng.integers(0, 2, 60)
    assert 0 < pale.sum() < 60
    retina = Retina(id_map=id_map, pale_mask=pale)
    imgs = rng.integers(0, 256, size=(4, 27, 912, 3), dtype=np.uint8)
    # the chunks of the second two-chunk iteration (1024..1026 with 1536..1538) in bytes no other chunk holds
    imgs[1] = 0
    imgs[1].reshape(1539, 16, 3)[[1024, 1025, 1026, 1536, 1537, 1538]] = 255
    imgs[2] = 255
    _check(torch_mod, retina, imgs)


def test_plain_kernel_stops_at_the_last_chunk(torch_mod):
    """The same 1539 chunks through the ABI itself, from buffers that go on for one more chunk: 16 pixels of ommatidium 1 behind
    the id map, 48 bytes of 255 behind the last image.  A loop that took chunk 1539 would add them (for the other images: the
    first 16 pixels of the next image) to ommatidium 1 without leaving the buffers."""
    torch = torch_mod
    import ctypes
    import sensors_oracle as so
    from flygym_amd import _native

    rng = np.random.default_rng(12)
    n_pix, n_omm = 16 * 1539, 60
    id_map = _run_map(rng, (27, 912), n_omm, lambda k: int(rng.integers(1, 41)))
    pale = rng.integers(0, 2, n_omm).astype(np.uint8)
    pale[0] = 0
    counts = np.bincount(id_map.ravel(), minlength=n_omm + 1)[1:]
    inv_norm = (1.0 / (255.0 * counts)).astype(np.float32)
    imgs = rng.integers(1, 256, size=(3, 27, 912, 3), dtype=np.uint8)          # (no byte 0: an extra chunk always adds)
    ids = id_map.ravel().astype(np.int64)
    typed = (ids | (np.where(ids > 0, pale[np.maximum(ids, 1) - 1], 0).astype(np.int64) << 15)).astype(np.uint16)
    id_dev = torch.as_tensor(np.concatenate([typed, np.full(16, 1, dtype=np.uint16)]).view(np.int16), device="cuda:0")
    img_dev = torch.as_tensor(np.concatenate([imgs.reshape(-1), np.full(48, 255, dtype=np.uint8)]), device="cuda:0")
    pale_dev, norm_dev = torch.as_tensor(pale, device="cuda:0"), torch.as_tensor(inv_norm, device="cuda:0")
    out = torch.full((3, n_omm, 2), -1.0, dtype=torch.float32, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
    _native.check(_native.lib().nmf_retina_resample(img_dev.data_ptr(), id_dev.data_ptr(), None, pale_dev.data_ptr(), norm_dev.data_ptr(),
                                                    3, n_pix, n_omm, out.data_ptr(), stream))
    want = so.retina_resample(imgs, id_map, pale, inv_norm)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n_group", [9, 16, 17])
def test_paired_groups_of_the_streaming_kernel(torch_mod, n_group):
    rng = np.random.default_rng(100 + n_group)
    shape = {9: (96, 96), 16: (128, 128), 17: (136, 128)}[n_group]
    assert shape[0] * shape[1] == 1024 * n_group
    id_map = _run_map(rng, shape, 40, _hostile_runs(rng))
    retina = Retina(id_map=id_map, pale_mask=rng.integers(0, 2, 40))
    imgs = rng.integers(0, 256, size=(5,) + shape + (3,), dtype=np.uint8)
    bands = imgs.reshape(5, n_group, 1024, 3)                      # a view: group g = pixels 1024 g .. 1024 g + 1023
    g = np.arange(n_group)
    # wave w pairs group g = w with group g + 8: the first eight groups all 0, their partners all 255, and the reverse
    bands[1] = np.where((g // 8) % 2 == 0, 0, 255).astype(np.uint8)[:, None, None]
    bands[2] = np.where((g // 8) % 2 == 0, 255, 0).astype(np.uint8)[:, None, None]
    bands[3] = ((37 * g + 11) % 256).astype(np.uint8)[:, None, None]   # every group its own byte
    got = _check(torch_mod, retina, imgs)
    assert not np.array_equal(got[1], got[2])


# the run structures of a 16-pixel chunk, by hand; ids 1..17, odd ids yellow and even ids pale (so both types are adjacent)
_HAND_CHUNKS = [
    [1] * 16,                                  # one run of one id
    [0] * 16,                                  # all background
    [2] * 8 + [3] * 8,                         # two runs
    [3] * 16,                                  # ... the second goes on to the chunk border and beyond it
    [4] * 16,                                  # a run that ends exactly on both borders
    [0] * 5 + [5] * 11,                        # two runs, background first
    [5] * 11 + [0] * 5,                        # two runs, background last
    [0] * 4 + [6] * 6 + [7] * 6,               # three runs, background in the first place
    [6] * 4 + [0] * 6 + [7] * 6,               # ... the second
    [6] * 4 + [7] * 6 + [0] * 6,               # ... the third
    [8] * 5 + [9] * 5 + [10] * 6,              # three runs, no background
    [1, 2, 3, 4] * 4,                          # sixteen runs
    [11] * 4 + [12] * 4 + [13] * 4 + [14] * 4,  # four runs
    [9] * 6 + [0] * 4 + [9] * 6,               # the same id on both sides of a background gap
    [9] * 3 + [0] * 2 + [9] * 3 + [0] * 8,     # ... and four runs of it
    [0] * 15 + [15],                           # one pixel at the end
    [15] + [0] * 15,                           # one pixel at the start
    [16] + [17] * 14 + [16],                   # a | b | a
    [2] * 15 + [3],
    [3] + [2] * 15,
    [12] * 15 + [0],
    [0] + [13] * 15,
    [10] * 8 + [11] * 7 + [12],                # three runs ending on the border, the last of one pixel
    [12] * 16,
]


def _hand_map(n_chunk, rng):
    """``n_chunk`` chunks: the hand-built ones, then random picks of them (so they meet in every order)."""
    chunks = list(_HAND_CHUNKS) + [_HAND_CHUNKS[int(k)] for k in rng.integers(0, len(_HAND_CHUNKS), n_chunk - len(_HAND_CHUNKS))]
    return np.array(chunks, dtype=np.int16).reshape(-1)


def _plan_words(typed):
    """The per-chunk plan words (comment above ``nmf_retina_plan_kernel``), from the runs of each chunk of typed ids."""
    words = np.zeros((typed.size // 16, 4), dtype=np.uint32)
    for ch, t in enumerate(typed.reshape(-1, 16).astype(np.uint32)):
        starts = [0] + [k for k in range(1, 16) if t[k] != t[k - 1]]           # first pixel of every run
        ida = int(t[0])
        idb, n1 = (int(t[starts[1]]), starts[1]) if len(starts) > 1 else (0, 16)
        idc, n2 = (int(t[starts[2]]), starts[2]) if len(starts) > 2 else (0, 16)
        more = 1 if len(starts) > 3 else 0
        palebits = sum(((int(t[k]) >> 15) & 1) << k for k in range(16))
        words[ch] = (ida | (idb << 16), idc | (more << 16), palebits, ((1 << n1) - 1) | (((1 << n2) - 1) << 16))
    return words


def _check_plan(torch, retina):
    """The plan blob the Retina built on the device == [plan words][ascending active chunks ...][count]."""
    id_dev, _, _, plan = retina._device_constants(torch, torch.device("cuda", 0))
    ids = retina.id_map.ravel().astype(np.int64)
    typed = (ids | (np.where(ids > 0, retina.pale_mask[np.maximum(ids, 1) - 1], 0).astype(np.int64) << 15)).astype(np.uint16)
    np.testing.assert_array_equal(id_dev.cpu().numpy().view(np.uint16), typed)
    n_chunk = typed.size // 16
    blob = plan.cpu().numpy()
    assert blob.size == n_chunk * 16 + ((n_chunk * 4 + 4 + 15) // 16) * 16
    words = blob[:n_chunk * 16].view(np.uint32).reshape(n_chunk, 4)
    want = _plan_words(typed)
    np.testing.assert_array_equal(words, want)
    tail = blob[n_chunk * 16:].view(np.int32)
    active = np.flatnonzero((ids.reshape(n_chunk, 16) != 0).any(axis=1))
    assert tail[n_chunk] == len(active)
    np.testing.assert_array_equal(tail[:len(active)], active)
    return want, active


def test_every_run_structure_of_a_chunk(torch_mod):
    rng = np.random.default_rng(5)
    pale = (np.arange(1, 18) % 2 == 0).astype(np.uint8)
    for shape in ((32, 32), (26, 40)):             # 64 chunks: the streaming kernel; 65 chunks: the plain one
        n_chunk = shape[0] * shape[1] // 16
        retina = Retina(id_map=_hand_map(n_chunk, rng).reshape(shape), pale_mask=pale)
        assert retina.num_ommatidia == 17
        imgs = rng.integers(0, 256, size=(4,) + shape + (3,), dtype=np.uint8)
        imgs[1] = 255
        imgs[2, :, :, 1], imgs[2, :, :, 2] = 1, 254                             # green and blue told apart
        _check(torch_mod, retina, imgs)
        words, active = _check_plan(torch_mod, retina)
        flagged = (words[:, 1] >> 16) & 1
        assert flagged[:len(_HAND_CHUNKS)].tolist() == [1 if i in (11, 12, 14) else 0 for i in range(len(_HAND_CHUNKS))]
        assert 1 not in active[:2] and 0 in active


def test_1024_ommatidia_fill_the_accumulator_and_1025_are_refused(torch_mod):
    torch = torch_mod
    from flygym_amd import _native

    rng = np.random.default_rng(3)
    ids = np.repeat(np.arange(1, 1025, dtype=np.int16), 2)
    full = Retina(id_map=ids.reshape(32, 64), pale_mask=rng.integers(0, 2, 1024))
    assert full.num_ommatidia == 1024
    imgs = np.full((4, 32, 64, 3), 255, dtype=np.uint8)
    imgs[3] = rng.integers(0, 256, size=(32, 64, 3), dtype=np.uint8)
    got = _check(torch, full, imgs)
    assert (got[:3].max(axis=-1) == np.float32(510) * full.inv_norm).all()
    ids = np.concatenate([np.repeat(np.arange(1, 1024, dtype=np.int16), 2), np.array([1024, 1025], dtype=np.int16)])
    over = Retina(id_map=ids.reshape(32, 64), pale_mask=rng.integers(0, 2, 1025))
    assert over.num_ommatidia == 1025
    with pytest.raises(_native.NativeError, match="n_ommatidia"):
        over.raw_image_to_hex_pxls(torch.as_tensor(imgs, device="cuda:0"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_check(torch, full, imgs), got)               # the process is still usable


def test_a_pixel_count_that_is_no_multiple_of_16_is_refused(torch_mod):
    torch = torch_mod
    from flygym_amd import _native

    rng = np.random.default_rng(4)
    id_map = _run_map(rng, (25, 41), 12, lambda k: int(rng.integers(1, 20)))
    retina = Retina(id_map=id_map, pale_mask=rng.integers(0, 2, 12))
    imgs = torch.as_tensor(rng.integers(0, 256, size=(3, 25, 41, 3), dtype=np.uint8), device="cuda:0")
    with pytest.raises(_native.NativeError, match="multiple of 16"):
        retina.raw_image_to_hex_pxls(imgs)
    assert _native.lib().nmf_retina_plan_bytes(25 * 41) == 0
    torch.cuda.synchronize()


def test_plan_blob_of_hostile_and_sparse_maps(torch_mod):
    rng = np.random.default_rng(17)
    hostile = Retina(id_map=_run_map(rng, (136, 128), 40, _hostile_runs(rng)), pale_mask=rng.integers(0, 2, 40))
    words, active = _check_plan(torch_mod, hostile)
    flagged = (words[:, 1] >> 16) & 1
    print(f"hostile map: {flagged.mean():.2f} of the chunks have more than three runs, {len(active)} of {len(words)} are active")
    assert 0.1 < flagged.mean() < 0.9 and len(active) > 1000       # three-run chunks and per-pixel chunks both occur
    # 808 chunks (three blocks of 256 and 40 more), the active ones unevenly spread: empty waves, full waves, a block with only
    # its first and last chunk, sparse and dense stretches
    n_chunk = 808
    p = np.zeros(n_chunk)
    p[64:128] = 1.0
    p[128:256] = 0.1
    p[256:320] = 1.0
    p[384:512] = 0.5
    p[[512, 767]] = 1.0
    p[768:] = 0.7
    on = rng.random(n_chunk) < p
    assert not on[:64].any() and on[64:128].all() and on[512:768].sum() == 2 and 0 < on[128:256].sum() < 40
    ids = np.zeros((n_chunk, 16), dtype=np.int16)
    for ch in np.flatnonzero(on):
        k = int(rng.integers(0, 16))
        ids[ch, k:k + int(rng.integers(1, 17))] = int(rng.integers(1, 21))
    ids[64, :] = 0
    ids[64, 15] = 1                                                   # (still active: one pixel)
    ids[65:85, 3] = np.arange(1, 21)                                  # every id occurs
    sparse = Retina(id_map=ids.reshape(16, n_chunk), pale_mask=rng.integers(0, 2, 20))
    _, active = _check_plan(torch_mod, sparse)
    assert len(active) == on.sum()
    imgs = rng.integers(0, 256, size=(3, 16, n_chunk, 3), dtype=np.uint8)
    _check(torch_mod, sparse, imgs)

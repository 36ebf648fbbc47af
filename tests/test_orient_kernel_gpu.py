"""odic_orient_rgb8 (csrc/orient.hip) against `Image.transpose`, bit for bit: every orientation at the shapes where the
tile walk changes, sources with a row pitch and odd offsets, mixed jobs in one launch, and a destination whose every
byte outside the outputs must keep its poison."""
import numpy as np
import pytest
import torch
from PIL import Image

import guards
from on_device_image_captioning_amd import jpeg as J
from on_device_image_captioning_amd.image_utils import ORIENT_JOB_DTYPE

pytestmark = pytest.mark.gpu

T = 64                                                                  # the kernel's tile side (csrc/orient.hip)
SHAPES = [(1, 1), (1, T + 1), (T + 1, 1), (T, T), (T - 1, T + 1), (2 * T + 3, T - 5), (5, 7)]
BAND = guards.MIN_BAND_BYTES
DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from on_device_image_captioning_amd import _hip
    return _hip, _hip.load()


def want(a, o):
    return np.asarray(Image.fromarray(a).transpose(J.transpose_method(o)))


def run(hip, jobs, seed=0):
    """jobs: [(H, W, orientation, pad bytes per source row, odd source offset?, gap in front of the output)].  One launch;
    every output compared, every other byte of the destination allocation checked for its poison."""
    _hip, lib = hip
    rng = np.random.default_rng(seed)
    rec = np.zeros(len(jobs), ORIENT_JOB_DTYPE)
    srcs, spos, dpos = [], BAND, BAND
    for r, (H, W, o, pad, s_odd, gap) in zip(rec, jobs):
        a = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        stride = 3 * W + pad
        spos += s_odd
        dpos += gap
        r["src_off"], r["dst_off"], r["src_stride_bytes"], r["H"], r["W"], r["orientation"] = spos, dpos, stride, H, W, o
        srcs.append(a)
        spos += H * stride
        dpos += 3 * H * W
    src = np.full(spos + BAND, guards.POISON, np.uint8)
    for r, a in zip(rec, srcs):
        H, W = a.shape[:2]
        rows = np.lib.stride_tricks.as_strided(src[int(r["src_off"]):], (H, 3 * W), (int(r["src_stride_bytes"]), 1))
        rows[:] = a.reshape(H, 3 * W)
    d_src = torch.from_numpy(src).to(DEV)
    d_dst = torch.full((dpos + BAND,), guards.POISON, dtype=torch.uint8, device=DEV)
    _hip.check(lib.odic_orient_rgb8(rec.ctypes.data, len(rec), d_src.data_ptr(), d_dst.data_ptr(), None),
               "odic_orient_rgb8")
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    outside = np.ones(got.size, bool)
    for r, a in zip(rec, srcs):
        lo, n = int(r["dst_off"]), a.size
        w = want(a, int(r["orientation"]))
        assert np.array_equal(got[lo:lo + n].reshape(w.shape), w), (a.shape, int(r["orientation"]), lo)
        outside[lo:lo + n] = False
    stray = np.flatnonzero(outside & (got != guards.POISON))
    assert stray.size == 0, f"stray write at byte {int(stray[0])} of the destination"
    assert torch.equal(d_src.cpu(), torch.from_numpy(src))             # the source is only read


@pytest.mark.parametrize("o", range(2, 9))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_every_orientation_at_the_tile_edges(hip, shape, o):
    run(hip, [(*shape, o, 0, 0, 0)])                                   # packed, 256-aligned
    run(hip, [(*shape, o, 5, 1, 3)], seed=1)                           # a view: pitch 3 W + 5, odd src_off and dst_off


@pytest.mark.parametrize("seed", [0, 1])
def test_mixed_jobs_in_one_launch(hip, seed):
    """Different sizes and orientations, odd gaps between the outputs, more tiles than jobs."""
    rng = np.random.default_rng(seed)
    jobs = [(H, W, 2 + (k + seed) % 7, int(rng.integers(0, 7)), int(rng.integers(0, 4)), int(rng.integers(1, 9)))
            for k, (H, W) in enumerate(SHAPES + [(3 * T + 1, 2 * T + 2), (2, 3 * T)])]
    run(hip, jobs, seed)


def test_more_jobs_than_one_launch_takes(hip):
    """65 jobs: the entry point sends 64 as kernel arguments and launches again for the rest."""
    run(hip, [(3 + k % 5, 2 + k % 7, 2 + k % 7, k % 3, k % 2, 1 + k % 4) for k in range(65)])


def test_nothing_to_do_and_refusals_write_nothing(hip):
    _hip, lib = hip
    dst = torch.full((4096,), guards.POISON, dtype=torch.uint8, device=DEV)
    src = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    rec = np.zeros(2, ORIENT_JOB_DTYPE)
    rec["src_stride_bytes"], rec["H"], rec["W"], rec["orientation"] = 21, 5, 7, 6
    rec["dst_off"][1] = 105
    assert lib.odic_orient_rgb8(rec.ctypes.data, 0, src.data_ptr(), dst.data_ptr(), None) == 0
    rec["orientation"][1] = 9                                           # the first job is fine: it must not run either
    assert lib.odic_orient_rgb8(rec.ctypes.data, 2, src.data_ptr(), dst.data_ptr(), None) == -1
    with pytest.raises(RuntimeError, match="ODIC_EINVAL"):
        _hip.check(lib.odic_orient_rgb8(rec.ctypes.data, 2, src.data_ptr(), dst.data_ptr(), None), "odic_orient_rgb8")
    torch.cuda.synchronize()
    assert bool((dst == guards.POISON).all())

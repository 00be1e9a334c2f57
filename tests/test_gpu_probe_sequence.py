"""GPU: the five probes one after another on one context.  They share the call frame of csrc/dct3d_probes.cpp and the
context's d_rate_tabs, d_rate_sums, pinned block, d_dist_sse, d_rate_bits, d_ssim_blk and d_ssim_part, so a stale
buffer or a stale size shows only when calls of different probes, sizes and table counts follow each other.  A fixed
interleaving of every probe, device- and host-pointer form, in every colour mode it accepts, with all optional outputs,
sizes going large -> small -> large and table counts 9 -> 1 -> 8 (two batches of kRateTables, one table, one full batch):
each result is bit-equal to the same call made first on a freshly created context."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def mode_on(ctx, pkg, mode):
    ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_PLANES if mode == "planes" else pkg.DCT3D_COLOUR_YCBCR)
    ctx.set_chroma(pkg.DCT3D_CHROMA_420 if mode == "c420" else pkg.DCT3D_CHROMA_444)
    try:
        yield ctx
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_PLANES)


# (w, h, stacks, tables): 17 x 9 has an edge, a 4:2:0 half row piece, 6 cubes and 8 windows per frame; 16 x 16 has none
PHASES = [(17, 9, 2, 9), (16, 16, 1, 1), (17, 9, 2, 8), (16, 16, 2, 9), (17, 9, 1, 1), (16, 16, 2, 8)]
# (probe, mode): grey is one channel; planes, ycc and c420 are packed RGB24 in the three colour modes
KINDS = [("rate", m) for m in ("grey", "planes", "ycc", "c420")] + \
        [(p, m) for p in ("distortion", "ssim") for m in ("grey", "planes")] + \
        [(p, m) for p in ("distortion_rgb", "ssim_rgb") for m in ("planes", "ycc", "c420")]
SPECS = [(p, m, host) for host in (False, True) for p, m in KINDS]
# neighbours in the sequence differ in probe, mode and form (11 is coprime to the 28 specs)
ORDER = [SPECS[(11 * i) % len(SPECS)] for i in range(len(SPECS))]


def frames(depth, w, h, stacks, channels):
    rng = np.random.default_rng(1000 * w + 10 * h + stacks + channels)
    shape = (stacks * depth, h, w) + ((3,) if channels == 3 else ())
    ramp = (np.arange(w)[None, None, :] * 5 + np.arange(h)[None, :, None] * 3).astype(np.int64)
    noise = rng.integers(0, 64, shape)
    return np.ascontiguousarray((noise + (ramp[..., None] if channels == 3 else ramp)) % 256, np.uint8)


def tables_of(pkg, depth, n):
    return [pkg.quant_table(q, depth) for q in ((5,) if n == 1 else range(10 - n, 10))]


def run_call(pkg, torch, ctx, depth, spec, phase):
    """one probe call with every optional output -> the list of its results as numpy arrays"""
    probe, mode, host = spec
    w, h, stacks, n = phase
    channels = 1 if mode == "grey" else 3
    fr = frames(depth, w, h, stacks, channels)
    tabs = tables_of(pkg, depth, n)
    cand = [(i, (i + 1) % n, (i + 2) % n) for i in range(n)]
    cps = ((w + 7) // 8) * ((h + 7) // 8)
    nwx, nwy = pkg.ssim_windows(w, h)
    luma = mode in ("ycc", "c420")
    dev = None

    def out(shape, dtype):
        nonlocal dev
        dev = torch.full(shape, 0x55, dtype=dtype, device="cuda")
        return dev

    with mode_on(ctx, pkg, "planes" if mode == "grey" else mode):
        if host:
            res = {"rate": lambda: ctx.rate_frames(fr, tabs),
                   "distortion": lambda: ctx.distortion_frames(fr, tabs, want_bits=True),
                   "ssim": lambda: ctx.ssim_frames(fr, tabs, want_sse=True, want_bits=True),
                   "distortion_rgb": lambda: ctx.distortion_rgb_frames(fr, tabs, cand, want_planes=True, want_bits=True),
                   "ssim_rgb": lambda: ctx.ssim_rgb_frames(fr, tabs, cand, want_luma=luma, want_sse=True, want_bits=True)}[probe]()
        else:
            d = torch.from_numpy(fr).cuda()
            if probe == "rate":  # (4:2:0: the cube layout is ragged, only the totals are offered)
                res = ctx.rate_frames_dev(d, w, h, channels, stacks, tabs,
                                          None if mode == "c420" else out((n, stacks, channels, cps), torch.int16))
            elif probe == "distortion":
                res = ctx.distortion_frames_dev(d, w, h, channels, stacks, tabs, out((n, stacks, channels, cps), torch.int32), want_bits=True)
            elif probe == "ssim":
                res = ctx.ssim_frames_dev(d, w, h, channels, stacks, tabs, out((n, stacks, channels, depth, nwy, nwx), torch.int32),
                                          want_sse=True, want_bits=True)
            elif probe == "distortion_rgb":
                res = ctx.distortion_rgb_frames_dev(d, w, h, stacks, tabs, cand, out((n, stacks, cps), torch.int32), want_planes=True,
                                                    want_bits=True)
            else:
                res = ctx.ssim_rgb_frames_dev(d, w, h, stacks, tabs, cand, out((n, 3, stacks, depth, nwy, nwx), torch.int32),
                                              want_luma=luma, want_sse=True, want_bits=True)
    res = [res] if isinstance(res, np.ndarray) else list(res)
    return res + ([dev.cpu().numpy()] if dev is not None else [])


def n_results(spec):
    """the host results with every optional one, the luma sums in the YCbCr modes, the device output of a _dev form"""
    probe, mode, host = spec
    n = {"rate": 1, "distortion": 2, "ssim": 3, "distortion_rgb": 3, "ssim_rgb": 3}[probe]
    return n + (probe == "ssim_rgb" and mode != "planes") + (not host and (probe, mode) != ("rate", "c420"))


def sequence():
    """every spec three times, in phases that go large -> small -> large (9 -> 1 -> 8 tables) from call to call"""
    return [(spec, PHASES[(i + r) % 3 + 3 * (r % 2)]) for r in range(3) for i, spec in enumerate(ORDER)]


@pytest.mark.parametrize("depth", [8, 4])
def test_interleaved_probes_equal_fresh_contexts(pkg, depth):
    import torch
    fresh = {}
    for spec, phase in sequence():
        if (spec, phase) not in fresh:
            ctx = pkg.Context(0, 8, 8, depth)
            try:
                fresh[spec, phase] = run_call(pkg, torch, ctx, depth, spec, phase)
            finally:
                ctx.close()
    assert len(fresh) == len(sequence())  # no call of the sequence repeats another
    ctx = pkg.Context(0, 8, 8, depth)
    try:
        for i, (spec, phase) in enumerate(sequence()):
            got, want = run_call(pkg, torch, ctx, depth, spec, phase), fresh[spec, phase]
            assert len(got) == len(want) == n_results(spec), (i, spec, phase)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.dtype == b.dtype and np.array_equal(a, b), f"call {i} {spec} {phase}: result {k}"
    finally:
        ctx.close()

"""GPU: the rate and distortion probes flag exactly what the host emulations flag.

rate_kernel (dct3d_rate.hip) and distortion_kernel (dct3d_distortion.hip) quantise and certify in loops of their
own, from table rows that probe-only host code builds per candidate table; at 8x8x8 the distortion probe transforms
with e16_forward, a hand copy of e16_body, and it runs the decode tile on LDS-staged integers with a reload source of
its own.  A certificate input that is slightly off changes no output on ordinary content: only the count of what was
left open sees it.  As test_gpu_certificates.py does for the encode and decode kernels, this module asserts exact
equality of dct3d_get_stats' n_flagged with cert_common.py's predictions, after the call's own result (bits and
squared error per cube and per stack) has been compared with the independent reference:

  rate probe        n_flagged = sum over the tables of the open coefficients (a coefficient open under k tables is
                    folded once and counted k times; the DC never; every geometry counts)
  distortion probe  n_flagged = sum over the tables of (the open coefficients + 32 x the lanes the decode tile
                    replays); the decode term is 0 at margin 0 (asserted on the CPU first), so the count at
                    margin 0 is the encode term alone

for the whole raster and for every band of one block row, per table set: each of ref, q1, q12, seeded alone, the
four in one call, and 11 tables (two launches per channel, so six launches for RGB: every launch adds into the one
counter slot and clears the other); at 1080p each of the 11 alone as well (cert_common.probe_sets).  The reference: quant_common's (the oracle's Java-semantics DCT and inverse with
the numpy quantiser around them -- ref_frames' composition, the DCT shared between a case's tables), code_bits for
the bits, test_gpu_distortion.cube_sums for the squared error."""
import functools

import numpy as np
import pytest

import cert_common as cc
import quant_common as qc
from cert_common import BIG_SUM, MARGINS, PROBE_CASES, PROBE_SETS
from conftest import ctx_option
from test_gpu_distortion import cube_sums

pytestmark = pytest.mark.gpu


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


def _cube_bits(q):
    """quant_common.code_bits summed per cube (through a table of code_bits over the cubes' value range)"""
    lo = int(q.min())
    lut = qc.code_bits(np.arange(lo, int(q.max()) + 1))
    return lut[q.reshape(q.shape[0], -1) - lo].sum(axis=1)


@functools.lru_cache(maxsize=None)
def _reference(c, name):
    """per (case, table), computed once: the reference's bits and squared error of every cube [stack, channel, cube],
    and the predicted terms per band and, last, for the whole raster: the open coefficients, the flagged lanes at
    each of PROBE_MARGINS"""
    T = cc.steps_of(cc.table(name, c.depth), c.depth)
    fr = c.frames()
    q = cc.case_q_ref(c, name)
    out = qc.ref_decode_frames(q, c.w, c.h, c.stacks, c.channels, T, c.depth)
    sse = cube_sums((fr.astype(np.int64) - out.astype(np.int64)) ** 2, c.depth)
    bits = _cube_bits(q).reshape(sse.shape)
    opens = cc.probe_open_counts(c, name)
    if name in c.rich:
        assert cc.is_rich(opens[:-1]), f"{c.id} {name} is not rich"
    lanes = {m: cc.probe_lane_counts(c, name, m) for m in cc.PROBE_MARGINS}
    assert lanes[0.0][-1] == 0, f"{c.id} {name}: the decode flags a lane at margin 0: another seed"
    for a in (sse, bits, opens) + tuple(lanes.values()):
        a.setflags(write=False)
    return {"sse": sse, "bits": bits, "open": opens, "lanes": lanes}


def _band(c, a, by):
    """[.., stack, channel, cube] of the whole raster -> the same of block row by (None: the whole raster)"""
    if by is None:
        return a
    nbx = a.shape[-1] // c.nby
    return a.reshape(a.shape[:-1] + (c.nby, nbx))[..., by, :]


def _tables(c, names):
    return [cc.steps_of(cc.table(n, c.depth), c.depth) for n in names]


def _calls(ctx, c, names, family, margin=0.0, want_bits=False):
    """the probe on every band and, last, on the whole raster, each result compared with the reference (per cube
    and per stack and channel) before its count is read: int64 [nby + 1]"""
    import torch
    refs = [_reference(c, n) for n in names]
    ref_bits, ref_sse = np.stack([r["bits"] for r in refs]), np.stack([r["sse"] for r in refs])
    tabs, fr, T = _tables(c, names), c.frames(), len(names)
    got = []
    for by in list(range(c.nby)) + [None]:
        f = fr if by is None else cc.band_frames(fr, by)
        rb, rs = _band(c, ref_bits, by), _band(c, ref_sse, by)
        h = f.shape[1]
        d_fr = torch.from_numpy(np.array(f)).cuda()
        n = rb.size * (2 if family == "rate" else 4)
        buf, mid = qc.banded(torch, n, 0xA5)
        where = f"{c.id} {family} band {by}"
        if family == "rate":
            bits = ctx.rate_frames_dev(d_fr, c.w, h, c.channels, c.stacks, tabs, mid)
            st = ctx.stats()
            cubes, intact = qc.bands_intact(buf, n, 0xA5)
            assert intact, f"{where}: a write outside d_cube_bits"
            assert np.array_equal(cubes.view(np.uint16).reshape(rb.shape).astype(np.int64), rb), f"{where}: cube bits"
        else:
            res = ctx.distortion_frames_dev(d_fr, c.w, h, c.channels, c.stacks, tabs, mid, want_bits)
            st = ctx.stats()
            sse, bits = res if want_bits else (res, None)
            cubes, intact = qc.bands_intact(buf, n, 0xA5)
            assert intact, f"{where}: a write outside d_cube_sse"
            assert np.array_equal(cubes.view(np.uint32).reshape(rs.shape).astype(np.int64), rs), f"{where}: cube sse"
            assert np.array_equal(sse.astype(np.int64), rs.sum(axis=-1)), f"{where}: the sums of the squared error"
        if bits is not None:
            assert np.array_equal(bits.astype(np.int64), rb.sum(axis=-1)), f"{where}: the sums of the bits"
        assert st["n_units"] == rb.size * 64 * c.depth, where
        got.append(int(st["n_flagged"]))
    return np.asarray(got, np.int64)


def _equal_counts(c, names, what, pred, got):
    """pred, got: per-band counts, the whole raster's last"""
    print(f"{c.id} {what}: predicted {int(pred[-1])}, device {int(got[-1])}")
    if not np.array_equal(pred[:-1], got[:-1]):
        mask = functools.reduce(np.logical_or, [cc.case_open(c, n)[1] for n in names])
        pytest.fail(f"{c.id} {what}: " + cc.first_difference(pred[:-1], got[:-1], mask, c.stacks, c.channels, c.nby) +
                    f"\npredicted per band {pred[:-1].tolist()}\ndevice per band {got[:-1].tolist()}")
    assert pred[-1] == got[-1], f"{c.id} {what}: the bands agree, the whole raster does not"


@pytest.mark.parametrize("c, tset", [(c, s) for c in PROBE_CASES for s in cc.probe_sets(c)],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_probe_counts(pkg, gpu_ctx8, gpu_ctx4, c, tset):
    """a: rate_frames_dev, count = sum of the open coefficients.  b: distortion_frames_dev at margin 0: the same
    count (e16_forward's statistics and coefficients, the probe's table rows).  c: at MARGINS[0] and MARGINS[1], with
    and without the bits: the decode tile's replays on top, and asking for the bits moves nothing.  (d: the RGB
    cases under the 11 tables are six launches into one counter slot.)"""
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names = PROBE_SETS[tset]
    refs = [_reference(c, n) for n in names]
    opens = sum(r["open"] for r in refs)
    assert np.array_equal(opens, cc.rate_probe_counts(c, names))
    if cc.probe_rich(c, tset):
        assert cc.is_rich(opens[:-1]), f"{c.id} {tset} is not rich"
    ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, 0)
    _equal_counts(c, names, f"{tset} rate", opens, _calls(ctx, c, names, "rate"))
    assert sum(int(r["lanes"][0.0][-1]) for r in refs) == 0  # (b): the encode term alone
    _equal_counts(c, names, f"{tset} distortion margin 0", opens, _calls(ctx, c, names, "distortion"))
    for m in MARGINS[:2]:
        pred = opens + 32 * sum(r["lanes"][m] for r in refs)
        for want_bits in (False, True):
            with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, m):
                got = _calls(ctx, c, names, "distortion", m, want_bits)
            _equal_counts(c, names, f"{tset} distortion margin {m} bits {want_bits}", pred, got)
        if cc.probe_rich(c, tset):
            assert pred[-1] > opens[-1] > 0  # both terms count


@pytest.mark.parametrize("depth", [8, 4])
def test_host_calls_count_as_the_device_calls(pkg, gpu_ctx8, gpu_ctx4, depth):
    """e: test_gpu_distortion.py::test_host_call_in_several_chunks' raster (40 frames of 1920 x 1080: two chunks of
    whole stacks on the host-pointer path of distortion_frames): the host calls' n_flagged is the device calls' on
    the whole raster, as n_units is -- no chunk's launches clear the slot the chunks before it counted into.  At
    MARGINS[0], so that both terms count."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 1920, 1080, 40 // depth
    fr = np.random.default_rng(20261020).integers(0, 256, (40, h, w), dtype=np.uint8)
    fr[8:16] //= 4
    tabs = _tables(cc.Case("uniform", depth, 1, w, h, stacks), ("q2", "q12"))
    d_fr = torch.from_numpy(fr).cuda()
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, MARGINS[0]):
        sse, bits = ctx.distortion_frames_dev(d_fr, w, h, 1, stacks, tabs, want_bits=True)
        dev = ctx.stats()
        hs, hb = ctx.distortion_frames(fr, tabs, want_bits=True)
        host = ctx.stats()
    assert np.array_equal(hs, sse) and np.array_equal(hb, bits)
    assert host["n_units"] == dev["n_units"] == 2 * fr.size
    print(f"distortion: device {dev['n_flagged']}, host {host['n_flagged']}")
    assert host["n_flagged"] == dev["n_flagged"] > 32 * stacks  # replays in every stack, and open coefficients
    rb = ctx.rate_frames_dev(d_fr, w, h, 1, stacks, tabs)
    dev = ctx.stats()
    hr = ctx.rate_frames(fr, tabs)
    host = ctx.stats()
    assert np.array_equal(rb, bits) and np.array_equal(hr, bits)
    assert host["n_units"] == dev["n_units"] == 2 * fr.size
    print(f"rate: device {dev['n_flagged']}, host {host['n_flagged']}")
    assert host["n_flagged"] == dev["n_flagged"] > 0


@pytest.mark.parametrize("depth", [8, 4])
def test_sums_past_2_32(gpu_ctx8, gpu_ctx4, depth):
    """distortion_sum_kernel adds uint64 partial sums sent as two 32-bit shuffles.  One grey stack of uniform noise
    under all255, large enough that the partial sum over 8 lanes is >= 2^32 in every 8-lane group of every wave
    (asserted from the reference's cube sums, by the kernel's partition: cert_common.sum_partials), so the high
    word's shuffles over 8, 16 and 32 lanes carry non-zero values: the stack's sum is the int64 sum of the returned
    cube map, and the map is the reference's."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = BIG_SUM[depth]
    fr = cc.content("uniform", depth, 1, w, h, 1)
    T = cc.steps_of(cc.table("all255", depth), depth)
    _, out = qc.ref_frames(fr, T, depth)
    ref = cube_sums((fr.astype(np.int64) - out.astype(np.int64)) ** 2, depth)  # [1, 1, C]
    part = cc.sum_partials(ref, 8)
    print(f"8x8x{depth} {w}x{h}: {ref.size} cubes, mean {ref.mean():.0f} per cube, least 8-lane partial "
          f"{int(part.min())} = {part.min() / 2.0 ** 32:.4f} x 2^32")
    assert part.size == 32 and part.min() >= 2 ** 32, "the frame is too small for the high word to travel"
    assert cc.sum_partials(ref, 1).max() < 2 ** 32  # a thread's own sum fits: the shuffles make the high word
    n = ref.size * 4
    buf, mid = qc.banded(torch, n, 0xA5)
    sse = ctx.distortion_frames_dev(torch.from_numpy(np.array(fr)).cuda(), w, h, 1, 1, [T], mid)
    cubes, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_cube_sse"
    cubes = cubes.view(np.uint32).astype(np.int64)
    assert sse.shape == (1, 1, 1) and int(sse[0, 0, 0]) == int(cubes.sum()) >= 2 ** 32
    assert np.array_equal(cubes, ref.reshape(-1)), f"{(cubes != ref.reshape(-1)).sum()} cubes differ from the reference"

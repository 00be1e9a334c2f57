"""GPU: the stream decode on periodic streams, whose wrong parses never fall into step.

The decode's front assumes that a parse begun at a chunk's first bit meets the true parse within a few codes.
`010010...` (all values 1) entered off a code boundary reads `1`, `00100`, `1`, ... for ever: the resolve walk ends
unmet, the speculative front reports an unresolved pass 0, and the rerun's confirming passes carry the correction
along the stream.  test_eg_sync_common.py proves what each stream below is (the host model, eg_sync_common.py); here
every entry point must give the reference's values, raster and end bit on them, and the front's sync launches
(Context.eg_sync_launches) must stay within ceil(n_chunks / 256) + 3 where a plain scheme takes one per chunk.

Streams are the oracle's writer's (test_gpu_eg._expected); rasters are compared with the oracle's decode of q."""
import numpy as np
import pytest

import eg_sync_common as m
from conftest import ctx_option
from test_gpu_eg import _expected
from test_gpu_eg_fused import _stream_dev

pytestmark = pytest.mark.gpu

W, H = 64, 40                       # 40 cubes per stack
PATTERNS = {"all1": 1, "alt1m1": (1, -1), "all2": 2, "all7": 7}
_CASES = {}


def _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4):
    return (gpu_ctx8, plan8) if depth == 8 else (gpu_ctx4, plan4)


def _case(key, pkg, oracle, plan, depth, vals, w=W, h=H, carry=(0, 0)):
    """(q, stream bytes, total bits, the reference's raster) of the values, made once and read-only"""
    key = (key, depth, w, h, carry)
    if key not in _CASES:
        q = m.cubes_of(vals, pkg.diagonal_order(8, 8, depth), depth)
        data, nbits = _expected(oracle, pkg, q, depth, *carry)
        ref = plan.decode_q(q, w, h, depth * (q.shape[0] // ((w // 8) * (h // 8))))
        for a in (q, ref):
            a.setflags(write=False)
        _CASES[key] = (q, data, nbits, ref)
    return _CASES[key]


def _counts(ctx):
    st = ctx.stats()
    return st["n_units"], st["n_flagged"], st["n_rechecked"]


def _two_step(ctx, data, n_cubes, start_bit=0):
    """dct3d_eg_decode_dev: (q, end bit, sync launches)"""
    import torch
    dq = torch.zeros(n_cubes * ctx.cube_size, dtype=torch.int32, device="cuda")
    eb = ctx.eg_decode_dev(_stream_dev(data), len(data), start_bit, n_cubes, dq)
    launches = ctx.eg_sync_launches()
    ctx.synchronize()
    return dq.cpu().numpy().reshape(n_cubes, ctx.bd, 8, 8), eb, launches


def _fused(ctx, data, w, h, stacks, start_bit=0):
    """dct3d_decode_eg_dev: (raster, end bit, sync launches, statistics)"""
    import torch
    out = torch.zeros((stacks * ctx.bd, h, w), dtype=torch.uint8, device="cuda")
    eb = ctx.decode_eg_dev(_stream_dev(data), len(data), start_bit, w, h, stacks, out)
    launches = ctx.eg_sync_launches()
    ctx.synchronize()
    return out.cpu().numpy(), eb, launches, _counts(ctx)


def _check_both(ctx, case, w, h, start_bit, lo, hi, what):
    """both device entry points on the stream, the fused one twice: the reference's results, the launches of each
    front in [lo, hi], the statistics those of the same call repeated"""
    q, data, nbits, ref = case
    stacks = q.shape[0] // ((w // 8) * (h // 8))
    got_q, eb, lq = _two_step(ctx, data, q.shape[0], start_bit)
    print(f"{what}: eg_decode_dev launches {lq}, allowed [{lo}, {hi}]")
    assert eb == nbits and np.array_equal(got_q, q)
    got, eb, lf, st = _fused(ctx, data, w, h, stacks, start_bit)
    print(f"{what}: decode_eg_dev launches {lf}")
    assert eb == nbits and np.array_equal(got, ref)
    again, eb2, lf2, st2 = _fused(ctx, data, w, h, stacks, start_bit)
    assert eb2 == nbits and np.array_equal(again, ref) and (lf2, st2) == (lf, st)
    assert st[0] == q.size                        # the rerun does not count the call's values twice
    for mx, sm in (lq, lf):
        assert mx == sm and lo <= mx <= hi, (what, lq, lf, lo, hi)
    return lq, lf


HOW = {"default": (None, 0), "fused front": ("DCT3D_OPT_EG_FUSED_FRONT", 0), "no resolve": ("DCT3D_OPT_EG_NO_RESOLVE", 0),
       "start bit 3": (None, 3)}


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("depth", [8, 4])
def test_never_meeting_streams(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, pattern, how):
    """All 1, (1, -1), all 2, all 7 at 64 x 40 x 1 stack (all 7 at 8x8x8: 280 chunks, two blocks of the chained pass;
    the others one), through the two-step and the fused call, by default, with the one-launch front, with plain
    passes from pass 0 on, and at start bit 3 behind a carried byte.  The front reruns (at least 3 launches: pass 0,
    a confirming pass that changes exits, one that does not) and stays within ceil(n_chunks / 256) + 3; a plain
    confirming pass per launch takes n_chunks of them (test_eg_sync_common.py)."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    option, start_bit = HOW[how]
    vals = m.periodic_values(PATTERNS[pattern], 40 * 64 * depth)
    case = _case(pattern, pkg, oracle, plan, depth, vals, carry=(0xA5, start_bit))
    hi = m.launch_bound(len(case[1]), start_bit)
    if option:
        with ctx_option(ctx, getattr(pkg, option), 1):
            _check_both(ctx, case, W, H, start_bit, 3, hi, f"{pattern} d{depth} {how}")
    else:
        _check_both(ctx, case, W, H, start_bit, 3, hi, f"{pattern} d{depth} {how}")


@pytest.mark.parametrize("depth,run,first", m.CHAINS)
def test_chain_of_known_length(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, run, first):
    """Random values with one run of 1s over 1, 2 or 5 whole chunks, out of step at its first: the model's plain
    scheme takes run + 1 confirming passes.  The device may take no more launches than that scheme behind the
    speculative attempt: its pass 0, the rerun's pass 0, those passes."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    vals = m.chain_case(depth, run, first)
    case = _case(("chain", run, first), pkg, oracle, plan, depth, vals)
    passes = m.FrontModel(case[1]).plain_passes()[0]
    assert passes == run + 1
    hi = min(2 + passes, m.launch_bound(len(case[1])))
    _check_both(ctx, case, W, H, 0, 1, hi, f"chain of {run} at {first} d{depth}")


@pytest.mark.parametrize("depth", [8, 4])
def test_late_meeting_takes_no_rerun(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth):
    """Runs of 1s across the first bit of every fourth chunk: there the walk ends unmet at 128 bits, the chunk's
    inline parse runs and gives the pass-0 exit again (the parses meet past bit 200, inside the chunk): exactly one
    sync launch, no rerun."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    case = _case("late", pkg, oracle, plan, depth, m.late_case(depth))
    f = m.FrontModel(case[1])
    assert f.plain_passes() == (1, f.n_chunks) and 4 * int((f.meeting_bits() > m.MEET_BITS).sum()) >= f.n_chunks
    _check_both(ctx, case, W, H, 0, 1, 1, f"late meeting d{depth}")


@pytest.mark.parametrize("value,w,h,stacks", [(0, 64, 40, 7), (-1, 64, 24, 4)])
@pytest.mark.parametrize("depth", [8, 4])
def test_in_step_runs_take_one_launch(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, value, w, h, stacks):
    """All 0 (every bit a code) and all -1 (`011`) over two blocks of chunks (280 and 288): every chunk is in step,
    every walk a run of 1-bit codes; nearly every chunk of a block walks at once.  One launch."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    stacks = stacks * 8 // depth
    vals = m.periodic_values(value, (w // 8) * (h // 8) * stacks * 64 * depth)
    case = _case(("in step", value), pkg, oracle, plan, depth, vals, w, h)
    assert m.FrontModel(case[1]).n_chunks > m.CHAIN_BLOCK
    _check_both(ctx, case, w, h, 0, 1, 1, f"all {value} d{depth}")


def _rgb_decode(ctx, streams, w, h, stacks):
    """dct3d_decode_eg_frames_dev on three streams: (frames [F, h, w, 3], end bits, sync launches)"""
    import torch
    out = torch.zeros((stacks * ctx.bd, h, w, 3), dtype=torch.uint8, device="cuda")
    eb = ctx.decode_eg_frames_dev([_stream_dev(b) for b in streams], [len(b) for b in streams], [0, 0, 0], w, h, stacks, out)
    launches = ctx.eg_sync_launches()
    ctx.synchronize()
    return out.cpu().numpy(), eb, launches


def _check_launches3(launches, bounds, what):
    """three fronts: each reruns when one must, each verdict and count its own"""
    mx, sm = launches
    print(f"{what}: launches max {mx}, sum {sm}, allowed per front {bounds}")
    assert 3 <= mx <= max(bounds) and mx + 2 <= sm <= sum(bounds), (what, launches, bounds)


@pytest.mark.parametrize("rotation", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 4])
def test_rgb24_planes_each_front_its_own_verdict(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, rotation):
    """Three streams at 24 x 16 x 2 stacks: all 7 (never meeting), random, all 0, and the two rotations: the front of
    the never-meeting channel reruns to its bound, the others take their own few launches."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    w, h, stacks = 24, 16, 2
    n = 6 * stacks * 64 * depth
    kinds = [("all7", m.periodic_values(7, n)), ("random", m.random_values(n, 31 + depth)), ("all0", m.periodic_values(0, n))]
    cases = [_case(("rgb", k), pkg, oracle, plan, depth, v, w, h) for k, v in kinds]
    cases = cases[rotation:] + cases[:rotation]
    got, eb, launches = _rgb_decode(ctx, [c[1] for c in cases], w, h, stacks)
    assert eb == [c[2] for c in cases]
    assert np.array_equal(got, np.stack([c[3] for c in cases], axis=-1))
    _check_launches3(launches, [m.launch_bound(len(c[1])) for c in cases], f"rgb24 planes d{depth} rotation {rotation}")


@pytest.mark.parametrize("periodic", ["Y", "chroma"])
@pytest.mark.parametrize("depth", [8, 4])
def test_rgb24_420_regions_of_different_lengths(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, periodic):
    """4:2:0 at 24 x 16 x 2 stacks: the Y stream over 12 cubes, the chroma streams over the 4 cubes of the padded
    12 x 8 planes; the Y stream all 7 and the chroma streams random, then the reverse."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    w, h, stacks = 24, 16, 2
    ny, nc = 6 * stacks * 64 * depth, 2 * stacks * 64 * depth
    seven = periodic == "Y"
    y = _case(("420 y", seven), pkg, oracle, plan, depth, m.periodic_values(7, ny) if seven else m.random_values(ny, 41), w, h)
    cb, cr = (_case(("420 c", seven, k), pkg, oracle, plan, depth,
                    m.random_values(nc, 43 + k) if seven else m.periodic_values(7, nc), 16, 8) for k in (0, 1))
    ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)
    ctx.set_chroma(pkg.DCT3D_CHROMA_420)
    try:
        got, eb, launches = _rgb_decode(ctx, [y[1], cb[1], cr[1]], w, h, stacks)
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, 0)
    assert eb == [y[2], cb[2], cr[2]]
    assert np.array_equal(got, pkg.ycbcr420_to_rgb(y[3], cb[3][:, :8, :12], cr[3][:, :8, :12]))
    _check_launches3(launches, [m.launch_bound(len(c[1])) for c in (y, cb, cr)], f"4:2:0 d{depth} periodic {periodic}")


@pytest.mark.parametrize("depth,stacks", [(8, 5), (4, 9)])
def test_host_pointer_chunks(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth, stacks):
    """dct3d_decode_eg at 24 x 16: the consumer runs in chunks of stacks (test_host_decode_eg_chunks_on_groups)
    behind a front that reran; all 7."""
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    for start_bit in (0, 5):
        q, data, nbits, ref = _case("host", pkg, oracle, plan, depth, m.periodic_values(7, 6 * stacks * 64 * depth), 24, 16,
                                    carry=(0xA5, start_bit))
        got, eb = ctx.decode_eg(data, 24, 16, stacks, start_bit=start_bit)
        mx, sm = ctx.eg_sync_launches()
        print(f"host pointer d{depth} start bit {start_bit}: launches {mx}")
        assert eb == nbits and np.array_equal(got, ref)
        assert mx == sm and 3 <= mx <= m.launch_bound(len(data), start_bit)


@pytest.mark.parametrize("depth", [8, 4])
def test_back_to_back_calls_keep_their_own_verdicts(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth):
    """A never-meeting stream, a random one and the never-meeting one again on one context with no synchronisation
    in between: the alternating status words must not carry the rerun's verdict into the next call."""
    import torch
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    n = 40 * 64 * depth
    never = _case("all7", pkg, oracle, plan, depth, m.periodic_values(7, n), carry=(0xA5, 0))
    rand = _case("random", pkg, oracle, plan, depth, m.random_values(n, 51 + depth))
    order = [never, rand, never, rand]
    streams = [_stream_dev(c[1]) for c in order]
    outs = [torch.zeros((depth, H, W), dtype=torch.uint8, device="cuda") for _ in order]
    qs = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in order]
    ebs, launches = [], []
    for c, s, o in zip(order, streams, outs):
        ebs.append(ctx.decode_eg_dev(s, len(c[1]), 0, W, H, 1, o))
        launches.append(ctx.eg_sync_launches()[0])
    for c, s, o in zip(order, streams, qs):
        ebs.append(ctx.eg_decode_dev(s, len(c[1]), 0, 40, o))
        launches.append(ctx.eg_sync_launches()[0])
    ctx.synchronize()
    assert ebs == [c[2] for c in order] * 2
    for c, o, dq in zip(order, outs, qs):
        assert np.array_equal(o.cpu().numpy(), c[3])
        assert np.array_equal(dq.cpu().numpy().reshape(c[0].shape), c[0])
    hi = m.launch_bound(len(never[1]))
    assert m.FrontModel(rand[1]).plain_passes()[0] == 1
    assert launches[1] == launches[3] == launches[5] == launches[7] == 1, launches
    assert all(3 <= launches[i] <= hi for i in (0, 2, 4, 6)), launches


@pytest.mark.parametrize("depth", [8, 4])
def test_error_verdicts_on_never_meeting_streams(pkg, oracle, plan8, plan4, gpu_ctx8, gpu_ctx4, depth):
    """Truncated: DCT3D_ENODATA; 48 zero bits planted: DCT3D_EINVAL or DCT3D_ENODATA (the slicing of
    test_fused_decode_truncated_and_corrupt), through both device calls; what is there still decodes."""
    import torch
    ctx, plan = _ctx_plan(depth, gpu_ctx8, gpu_ctx4, plan8, plan4)
    q, data, nbits, ref = _case("all7", pkg, oracle, plan, depth, m.periodic_values(7, 40 * 64 * depth), carry=(0xA5, 0))
    bad = bytearray(data)
    bad[len(bad) // 3: len(bad) // 3 + 6] = bytes(6)
    for stream, codes in ((data[: len(data) // 2], (pkg.DCT3D_ENODATA,)), (bytes(bad), (pkg.DCT3D_EINVAL, pkg.DCT3D_ENODATA))):
        with pytest.raises(pkg.Dct3dError) as e:
            _two_step(ctx, stream, 40)
        assert e.value.code in codes
        assert ctx.eg_sync_launches()[0] <= m.launch_bound(len(stream))
        with pytest.raises(pkg.Dct3dError) as e:
            _fused(ctx, stream, W, H, 1)
        assert e.value.code in codes
        assert ctx.eg_sync_launches()[0] <= m.launch_bound(len(stream))
        ctx.synchronize()
    got, eb, _ = _two_step(ctx, data[: len(data) // 2 + len(data) // 8], 20)       # half the cubes are there
    assert np.array_equal(got, q[:20]) and eb == nbits // 2
    got, eb, _, _ = _fused(ctx, data, W, H, 1)                                      # and the call after is good
    assert eb == nbits and np.array_equal(got, ref)

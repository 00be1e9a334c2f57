#!/usr/bin/env python3
"""A quantiser table per (stack, channel) in the fused stream calls (dct3d_*_eg_frames_vqc*) against the
per-stack _vq calls of the same build and of the parent commit, on device-resident 1080p RGB stacks (bench.py, the
flagship measurement, is not involved).

Per depth (8 x 8 x 8, 8 x 8 x 4), colour mode (4:4:4 YCbCr, 4:2:0) and direction (encode; decode of the streams that
encode wrote):
  (a)  the _vqc call with three distinct constant columns (0, 1, 2) over a palette whose first three tables are the
       SAME table (the reference's): the work and the streams are (b)'s, so a / b is what the channel axis costs
  (a') the _vqc call with three distinct tables, q = 5, 12, 20 for Y, Cb, Cr: what a caller would ask for (fewer bits
       in the chroma streams: no like-for-like figure)
  (b)  the _vq call of this build with one constant column
  (c)  the _vq call of the parent commit's build (--parent: a tree made by tools/ab_build.sh), in the same process, on
       the same stream, in rounds alternating with (b)
b / c must lie inside the spread that (c)'s own rounds show (min / median .. max / median); both are reported.

Content: `--stacks` (16; 42 is bench_c420's) packed RGB24 stacks of 1920 x 1080 of uniform noise or ramp (three
dct3d_fill_synthetic_dev planes of different seeds, interleaved: bench_ycc.py's).  Everything runs on one stream shared by
torch and the contexts, timed with device events; each variant is warmed up, then `--rounds` rounds alternate the
variants, `--iters` timed calls each, a round's figure being the median.  (a)'s streams are checked against (b)'s
before timing.  Prints one JSON document; --out also writes it to a file."""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def load_parent(tree):
    """the parent commit's package from its own tree, under a name of its own (it loads its own libdct3d.so)"""
    init = os.path.join(tree, "3ddctvideoencoding_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("dct3d_parent", init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["dct3d_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--kind", default="uniform")
    ap.add_argument("--stacks", type=int, default=16)
    ap.add_argument("--depths", default="8,4")
    ap.add_argument("--rounds", type=int, default=31)  # (7 were too few for the spread of (c)'s rounds: DESIGN 4r)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit (tools/ab_build.sh HEAD~1 base -> ab/base)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vqc.py needs a HIP device")
    parent = load_parent(os.path.abspath(a.parent)) if a.parent else None
    assert parent is None or os.path.realpath(parent.LIB_PATH) != os.path.realpath(pkg.LIB_PATH)
    n = a.stacks
    W, H = (int(v) for v in a.size.split("x"))
    CW, CH = pkg.chroma_size(W, H)
    stream = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(a.iters):
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms)

    def run_rounds(variants):
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        stream.synchronize()
        rounds = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():  # alternate the variants within a round
                rounds[k].append(round(timed(fn), 4))
        return rounds

    def make_ctx(p, D, mode):
        c = p.Context(0, 8, 8, D)
        c.set_stream(stream.cuda_stream)
        c.set_option(p.DCT3D_OPT_COLOUR, p.DCT3D_COLOUR_YCBCR)
        if mode == "420":
            c.set_chroma(p.DCT3D_CHROMA_420)
        return c

    import numpy as np
    cases = []
    with torch.cuda.stream(stream):
        for D in (int(d) for d in a.depths.split(",")):
            cs, F = 64 * D, n * D
            fill = pkg.Context(0, 8, 8, D)
            fill.set_stream(stream.cuda_stream)
            pl = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
            fill.fill_synthetic_dev(pl[0], W, H, F, kind=a.kind)
            fill.fill_synthetic_dev(pl[1], W, H, F, seed=0x77A1, frame0=3, kind=a.kind)
            fill.fill_synthetic_dev(pl[2], W, H, F, seed=0x51DE5, frame0=11, kind=a.kind)
            d_fr = pl.permute(1, 2, 3, 0).contiguous()
            del pl
            fill.close()
            ref = pkg.quant_table(5, D)
            pal = np.stack([ref, ref, ref, pkg.quant_table(12, D), pkg.quant_table(20, D)]).astype(np.int32)
            m_same = np.ascontiguousarray(np.broadcast_to(np.array([0, 1, 2], np.uint8), (n, 3)))
            m_dist = np.ascontiguousarray(np.broadcast_to(np.array([0, 3, 4], np.uint8), (n, 3)))
            col = np.zeros(n, np.uint8)
            for mode in ("444", "420"):
                sizes = [(W, H)] + [(CW, CH) if mode == "420" else (W, H)] * 2
                caps = [(-(-w // 8)) * (-(-h // 8)) * n * cs + 64 for w, h in sizes]  # bytes per stream: 8 bits per value
                keys = ["a", "a2", "b"] + (["c"] if parent else [])
                ctx = {k: make_ctx(parent if k == "c" else pkg, D, mode) for k in keys}
                d_s = {k: [torch.zeros(c // 4 + 1, dtype=torch.int32, device="cuda") for c in caps] for k in keys}
                d_out = {k: torch.empty_like(d_fr) for k in keys}
                bits = {}

                def enc(k):
                    if k in ("a", "a2"):
                        bits[k] = ctx[k].encode_eg_frames_vqc_dev(d_fr, W, H, 3, n, pal, m_same if k == "a" else m_dist, d_s[k], caps)
                    else:
                        bits[k] = ctx[k].encode_eg_frames_vq_dev(d_fr, W, H, 3, n, pal, col, d_s[k], caps)

                def dec(k):
                    nb = [(b + 7) // 8 for b in bits[k]]
                    if k in ("a", "a2"):
                        ctx[k].decode_eg_frames_vqc_dev(d_s[k], nb, [0] * 3, W, H, n, pal, m_same if k == "a" else m_dist, d_out[k])
                    else:
                        ctx[k].decode_eg_frames_vq_dev(d_s[k], nb, [0] * 3, W, H, n, pal, col, d_out[k])

                for k in keys:
                    enc(k)
                    dec(k)
                stream.synchronize()
                equal = all(bits[k] == bits["b"] and bool(torch.equal(d_out[k], d_out["b"])) and all(
                    bool(torch.equal(x[:(b + 31) // 32], y[:(b + 31) // 32])) for x, y, b in zip(d_s[k], d_s["b"], bits["b"]))
                    for k in keys if k != "a2")
                names = {"a": "a_vqc_same_tables", "a2": "a_vqc_q5_q12_q20", "b": "b_vq", "c": "c_vq_parent"}
                variants = {}
                for k in keys:
                    variants["enc_" + names[k]] = (lambda k=k: enc(k))
                for k in keys:
                    variants["dec_" + names[k]] = (lambda k=k: dec(k))
                rounds = run_rounds(variants)
                med = {k: statistics.median(v) for k, v in rounds.items()}
                case = {"depth": D, "chroma": mode, "size": a.size, "kind": a.kind, "stacks": n, "frame_bytes": d_fr.numel(),
                        "stream_bits": {names[k]: bits[k] for k in keys}, "ms_per_round": rounds, "ms_median": med,
                        "a_and_c_equal_b": equal}
                for d in ("enc", "dec"):
                    b_med = med[d + "_b_vq"]
                    case[d + "_a_over_b"] = round(med[d + "_a_vqc_same_tables"] / b_med, 4)
                    case[d + "_a2_over_b"] = round(med[d + "_a_vqc_q5_q12_q20"] / b_med, 4)
                    if parent:
                        c_r = rounds[d + "_c_vq_parent"]
                        c_med = med[d + "_c_vq_parent"]
                        case[d + "_b_over_c"] = round(b_med / c_med, 4)
                        case[d + "_c_spread"] = [round(min(c_r) / c_med, 4), round(max(c_r) / c_med, 4)]
                        case[d + "_b_over_c_inside_c_spread"] = min(c_r) / c_med <= b_med / c_med <= max(c_r) / c_med
                cases.append(case)
                for c in ctx.values():
                    c.close()
                del d_s, d_out
                torch.cuda.empty_cache()
            del d_fr
            torch.cuda.empty_cache()

    res = {"tool": "bench_vqc", "iters": a.iters, "rounds": a.rounds, "parent": bool(parent),
           "content": "three dct3d_fill_synthetic_dev planes (default seed; seed 0x77A1, frame0 3; seed 0x51DE5, frame0 11), interleaved",
           "cases": cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not all(c["a_and_c_equal_b"] for c in cases):
        raise SystemExit("the _vqc call with equal tables, the parent's _vq call and this build's _vq call differ")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused stream calls for frames of any size and packed RGB24 (encode_eg_frames_dev / decode_eg_frames_dev)
against what a caller had before them, on device-resident stacks of common screen sizes (bench.py, the flagship
measurement, is not involved).

  (a) the new call: frames -> one Exp-Golomb stream per channel, and back, no int32 intermediate
  (b) the parent commit's way for the same frames: encode = encode_frames_dev + eg_encode_dev over all the
      cubes; decode = eg_decode_dev + decode_frames_dev.  The same work, the order of the cubes in the stream
      aside (one stream over [stack][channel][cube]).  --parent DIR runs (b) in the library of a parent checkout
      built there (DIR holds its 3ddctvideoencoding_amd package; tools/ab_build.sh makes one), loaded beside
      this build's; without it (b) runs the same calls of this build.
  (c) the existing fused call (encode_eg_dev / decode_eg_dev) on grey content of the padded size with the same
      number of cubes (RGB: 3 x the stacks): the ceiling

Content 8 x 8 x 8 (or --depth 4), ramp and uniform; grey (126 stacks) and packed RGB24 (42 stacks).  Everything
runs on one stream shared by torch and the contexts, timed with device events; each case is warmed up, then
`--rounds` rounds alternate the variants, `--iters` timed calls each, the round's figure being the median.  Before
timing, (a)'s decode of (a)'s streams is compared with (b)'s decode of (b)'s stream, bit for bit.  Prints one JSON
document; --out also writes it to a file.

  --only enc|dec   for a profiler run of its own: untimed, `--iters` calls of (a) of the first --sizes entry, the
                   first --channels entry and the first --kinds entry
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def load_parent(path):
    """the package of another checkout under a name of its own (its library loads beside this build's)"""
    pdir = os.path.join(os.path.abspath(path), "3ddctvideoencoding_amd")
    spec = importlib.util.spec_from_file_location("dct3d_parent", os.path.join(pdir, "__init__.py"),
                                                  submodule_search_locations=[pdir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["dct3d_parent"] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1366x768,1680x1050,1920x1080")
    ap.add_argument("--channels", default="1,3")
    ap.add_argument("--kinds", default="ramp,uniform")
    ap.add_argument("--grey-stacks", type=int, default=126)
    ap.add_argument("--rgb-stacks", type=int, default=42)
    ap.add_argument("--depth", type=int, default=8, choices=(8, 4))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--only", default=None, choices=("enc", "dec"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_eg_frames.py needs a HIP device")
    D = a.depth
    cs = 64 * D
    stream = torch.cuda.Stream()
    ctx = pkg.Context(0, 8, 8, D)
    ctx.set_stream(stream.cuda_stream)
    ctx_b = ctx
    if a.parent:
        ctx_b = load_parent(a.parent).Context(0, 8, 8, D)
        ctx_b.set_stream(stream.cuda_stream)

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

    def content(W, H, C, n, kind):
        F = n * D
        if C == 1:
            t = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
            ctx.fill_synthetic_dev(t, W, H, F, kind=kind)
            return t
        planes = torch.empty((3, F, H, W), dtype=torch.uint8, device="cuda")
        ctx.fill_synthetic_dev(planes[0], W, H, F, kind=kind)
        ctx.fill_synthetic_dev(planes[1], W, H, F, seed=0x77A1, frame0=3, kind=kind)
        ctx.fill_synthetic_dev(planes[2], W, H, F, seed=0x51DE5, frame0=11, kind=kind)
        return planes.permute(1, 2, 3, 0).contiguous()

    cases = []
    with torch.cuda.stream(stream):
        for size in a.sizes.split(","):
            W, H = (int(v) for v in size.split("x"))
            Wp, Hp = pkg.padded_size(W, H)
            for C in (int(c) for c in a.channels.split(",")):
                for kind in a.kinds.split(","):
                    n = a.grey_stacks if C == 1 else a.rgb_stacks
                    n_cubes = ctx.n_cubes(Wp, Hp, n)  # per channel
                    d_fr = content(W, H, C, n, kind)
                    d_grey = content(Wp, Hp, 1, C * n, kind)  # (c): as many cubes, grey, padded size
                    cap = n_cubes * cs + 64               # bytes per channel: 8 bits per value
                    d_sa = [torch.zeros(cap // 4 + 1, dtype=torch.int32, device="cuda") for _ in range(C)]
                    d_sb = torch.zeros(C * cap // 4 + 1, dtype=torch.int32, device="cuda")
                    d_sc = torch.zeros(C * cap // 4 + 1, dtype=torch.int32, device="cuda")
                    d_q = torch.empty((C * n_cubes, D, 8, 8), dtype=torch.int32, device="cuda")
                    d_out_a = torch.empty_like(d_fr)
                    d_out_b = torch.empty_like(d_fr)
                    d_out_c = torch.empty_like(d_grey)
                    bits = {}

                    def enc_a():
                        bits["a"] = ctx.encode_eg_frames_dev(d_fr, W, H, C, n, d_sa, [cap] * C)

                    def enc_b():
                        ctx_b.encode_frames_dev(d_fr, W, H, C, n, d_q)
                        bits["b"] = ctx_b.eg_encode_dev(d_q, C * n_cubes, d_sb, C * cap)

                    def enc_c():
                        bits["c"] = ctx.encode_eg_dev(d_grey, Wp, Hp, C * n, d_sc, C * cap)

                    def dec_a():
                        ctx.decode_eg_frames_dev(d_sa, [(b + 7) // 8 for b in bits["a"]], [0] * C, W, H, n, d_out_a)

                    def dec_b():
                        ctx_b.eg_decode_dev(d_sb, (bits["b"] + 7) // 8, 0, C * n_cubes, d_q)
                        ctx_b.decode_frames_dev(d_q, W, H, C, n, d_out_b)

                    def dec_c():
                        ctx.decode_eg_dev(d_sc, (bits["c"] + 7) // 8, 0, Wp, Hp, C * n, d_out_c)

                    if a.only:
                        enc_a()
                        for _ in range(a.iters):
                            (enc_a if a.only == "enc" else dec_a)()
                        stream.synchronize()
                        print(json.dumps({"only": a.only, "size": size, "padded": f"{Wp}x{Hp}", "channels": C, "kind": kind,
                                          "stacks": n, "calls": a.iters + (1 if a.only == "enc" else 0),
                                          "frame_bytes": d_fr.numel(), "stream_bytes": [(b + 7) // 8 for b in bits["a"]]}))
                        ctx.close()
                        return
                    enc_a()
                    enc_b()
                    enc_c()
                    dec_a()
                    dec_b()
                    stream.synchronize()
                    equal = bool(torch.equal(d_out_a, d_out_b)) and sum(bits["a"]) == bits["b"]
                    rounds = run_rounds({"enc_a_new": enc_a, "enc_b_parent_int32": enc_b, "enc_c_ceiling": enc_c,
                                         "dec_a_new": dec_a, "dec_b_parent_int32": dec_b, "dec_c_ceiling": dec_c})
                    med = {k: statistics.median(v) for k, v in rounds.items()}

                    def kernel_split(fn):
                        """per call, from the context's own event pairs: the transform kernel(s) and the auxiliary
                        launches (encode: scan + compaction + stitch; RGB encode: the three chains summed)"""
                        stream.synchronize()
                        ctx.reset_timers()
                        ctx.set_profiling(True)
                        for _ in range(a.iters):
                            fn()
                        st = ctx.stats()
                        ctx.set_profiling(False)
                        return {"kernel_ms": round(st["kernel_ms_total"] / a.iters, 4), "aux_ms": round(st["aux_ms_total"] / a.iters, 4),
                                "timed_launch_groups_per_call": st["n_timed"] / a.iters}

                    split = {k: kernel_split(fn) for k, fn in (("enc_a_new", enc_a), ("enc_c_ceiling", enc_c),
                                                               ("dec_a_new", dec_a), ("dec_c_ceiling", dec_c))}
                    cases.append({
                        "kernel_split_per_call": split,
                        "size": size, "padded": f"{Wp}x{Hp}", "channels": C, "kind": kind, "stacks": n,
                        "frame_bytes": d_fr.numel(), "stream_bits": bits["a"], "ms_per_round": rounds, "ms_median": med,
                        "enc_a_over_b": round(med["enc_a_new"] / med["enc_b_parent_int32"], 4),
                        "enc_a_over_c": round(med["enc_a_new"] / med["enc_c_ceiling"], 4),
                        "dec_a_over_b": round(med["dec_a_new"] / med["dec_b_parent_int32"], 4),
                        "dec_a_over_c": round(med["dec_a_new"] / med["dec_c_ceiling"], 4),
                        "enc_a_faster_than_b_every_round": all(x < y for x, y in zip(rounds["enc_a_new"], rounds["enc_b_parent_int32"])),
                        "dec_a_faster_than_b_every_round": all(x < y for x, y in zip(rounds["dec_a_new"], rounds["dec_b_parent_int32"])),
                        "a_equals_b": equal,
                    })
                    del d_fr, d_grey, d_sa, d_sb, d_sc, d_q, d_out_a, d_out_b, d_out_c
                    torch.cuda.empty_cache()

    res = {"tool": "bench_eg_frames", "depth": D, "iters": a.iters, "rounds": a.rounds,
           "b_build": "parent checkout" if a.parent else "this build", "cases": cases}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()
    if ctx_b is not ctx:
        ctx_b.close()
    if not all(c["a_equals_b"] for c in cases):
        raise SystemExit("the new calls and the int32 route differ")


if __name__ == "__main__":
    main()

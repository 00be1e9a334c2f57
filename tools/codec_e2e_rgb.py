"""End-to-end timing of `dct3d_codec encode_rgb` / `decode_rgb` (run on the GPU box) on a synthetic packed RGB24
video whose size is no multiple of 8 (default 64 frames of 1366 x 768): this build (the fused stream calls: only the
frames and the streams cross PCIe) against DCT3D_CODEC_HOST_EG=1 (the int32 route, Exp-Golomb on the host) and,
with --parent DIR, against the dct3d_codec of another checkout built there (DIR/3ddctvideoencoding_amd/lib).  All
must write the same three files and the same decoded frames.  Every run reports its per-stage wall seconds
(DCT3D_CODEC_TIMING=1) where the build prints them.  Each command runs --repeat times; the figure is the
median.  One JSON document; --out also writes it to a file."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1366x768")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("3ddctvideoencoding_amd")
    W, H = (int(v) for v in a.size.split("x"))
    F = a.frames
    tmp = tempfile.mkdtemp(dir=os.environ.get("TMPDIR", "/tmp"))
    raw = os.path.join(tmp, "in.rgb")
    with open(raw, "wb") as f:
        for s in range(0, F, 8):
            n = min(8, F - s)
            planes = [pkg.synthetic.frames(W, H, n, kind="ramp", frame0=s),
                      pkg.synthetic.frames(W, H, n, seed=0x77A1, frame0=3 + s, kind="uniform"),
                      pkg.synthetic.frames(W, H, n, seed=0x51DE5, frame0=11 + s, kind="ramp")]
            f.write(np.stack(planes, axis=-1).tobytes())
    builds = {"this": (pkg.CLI_PATH, "0"), "this_host_eg": (pkg.CLI_PATH, "1")}
    if a.parent:
        builds["parent"] = (os.path.join(os.path.abspath(a.parent), "3ddctvideoencoding_amd", "lib", "dct3d_codec"), "0")
    res = {"tool": "codec_e2e_rgb", "size": a.size, "frames": F, "raw_MB": 3 * W * H * F / 1e6, "repeat": a.repeat, "runs": {}}

    def run(cli, cmd, src, dst, host_eg):
        env = dict(os.environ, DCT3D_CODEC_TIMING="1", DCT3D_CODEC_HOST_EG=host_eg)
        ts, stages = [], None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            r = subprocess.run([cli, cmd, src, dst, str(W), str(H), str(F), "1"], capture_output=True, text=True, env=env)
            ts.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stdout + r.stderr
            st = [json.loads(ln) for ln in r.stderr.splitlines() if ln.startswith('{"stage_s"')]
            stages = st[-1] if st else None
        return {"process_s": [round(t, 4) for t in ts], "process_s_median": round(statistics.median(ts), 4),
                "stages_last_run": stages}

    files, frames = {}, {}
    for name, (cli, he) in builds.items():
        enc = os.path.join(tmp, "enc_" + name)
        dec = os.path.join(tmp, "dec_" + name + ".rgb")
        res["runs"][name] = {"encode_rgb": run(cli, "encode_rgb", raw, enc, he), "decode_rgb": run(cli, "decode_rgb", enc, dec, he)}
        files[name] = [open(enc + sfx, "rb").read() for sfx in (".red", ".green", ".blue")]
        frames[name] = open(dec, "rb").read()
    res["stream_MB"] = sum(len(b) for b in files["this"]) / 1e6
    res["files_identical"] = all(v == files["this"] for v in files.values())
    res["decoded_identical"] = all(v == frames["this"] for v in frames.values())
    for cmd in ("encode_rgb", "decode_rgb"):
        for other in builds:
            if other != "this":
                res[f"{cmd}_this_over_{other}"] = round(res["runs"]["this"][cmd]["process_s_median"] /
                                                        res["runs"][other][cmd]["process_s_median"], 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not (res["files_identical"] and res["decoded_identical"]):
        raise SystemExit("the builds' files differ")


if __name__ == "__main__":
    main()

"""CPU: the probes' host arithmetic (csrc/dct3d_probe_layout.h) -- the SSIM geometry, the stacks per range and per
staging chunk, the table-to-slot compaction, the sections of the sums block and the index maps -- run by
tests/native/probe_layout_check.cpp (a stand-alone program under the address and undefined-behaviour sanitizers, one
child process for all queries) and compared with closed forms written here."""
import itertools
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (4, 4), (5, 3), (9, 4), (17, 9), (61, 45), (1366, 768), (1920, 1080)]
DEPTHS = [8, 4]
COUNTS = [1, 8, 9, 32]
SSIM_BUDGET, PLANE_BUDGET, CHUNK = 16 << 20, 64 << 20, 64 << 20


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = tmp_path_factory.mktemp("probe_layout") / "probe_layout_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "3ddctvideoencoding_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "probe_layout_check.cpp"), "-o", str(exe)], check=True)

    def ask(queries):
        """queries: lists of a command and integers -> one list of integers per query"""
        text = "".join(" ".join(str(v) for v in q) + "\n" for q in queries)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(queries)
        return [[int(v) for v in ln.split()] for ln in lines]
    return ask


def ceil_div(a, b):
    return -(-a // b)


def geom(w, h, D):
    nbx, nby = ceil_div(w, 4), ceil_div(h, 4)
    nwx, nwy = max(nbx - 1, 1), max(nby - 1, 1)
    return nbx, nby, nwx, nwy, D * nbx * nby, D * nwx * nwy


def test_ssim_geometry(ask, pkg):
    cases = [(w, h, D) for (w, h) in SIZES for D in DEPTHS] + [(2**31 - 1, 2**31 - 1, 8), (2**17 + 4, 2**16 + 4, 8), (2**17 + 4, 2**16 + 4, 4)]
    for (w, h, D), got in zip(cases, ask([("geom",) + c for c in cases])):
        nbx, nby, nwx, nwy, blk, win = geom(w, h, D)
        assert got == [nbx, nby, nwx, nwy, min(ceil_div(win, 1024), 1024), blk, win, int(win < 2**32)], (w, h, D)
        if w < 2**20:
            assert (nwx, nwy) == pkg.ssim_windows(w, h)
    assert geom(2**17 + 4, 2**16 + 4, 8)[5] == 2**32 and geom(2**17 + 4, 2**16 + 4, 4)[5] == 2**31  # the limit itself, and below it


def test_ssim_ranges(ask):
    """per size, depth and table count: the real budget, and budgets of exactly k stacks' records, one byte short of
    them, and short of a single stack's"""
    qs, want = [], []
    for (w, h), D, n, planes in itertools.product(SIZES, DEPTHS, COUNTS, (1, 3, 4)):
        rec = geom(w, h, D)[4] * (8 * n + 4) * planes
        for budget, n_stacks in [(SSIM_BUDGET, 7), (SSIM_BUDGET, 100000), (3 * rec, 7), (3 * rec - 1, 7), (3 * rec + rec - 1, 7),
                                 (rec - 1, 7), (3 * rec, 2), (rec, 1)]:
            qs.append(("ssimrange", budget, w, h, D, n, planes, n_stacks))
            want.append([rec, max(1, min(budget // rec, n_stacks, 65535))])
    got = ask(qs)
    assert got == want
    by_q = {q[1:]: g[1] for q, g in zip(qs, got)}
    rec = geom(17, 9, 8)[4] * (8 * 9 + 4)
    assert [by_q[b, 17, 9, 8, 9, 1, 7] for b in (3 * rec, 3 * rec - 1, 4 * rec - 1, rec - 1)] == [3, 2, 3, 1]
    assert by_q[SSIM_BUDGET, 1, 1, 8, 1, 1, 100000] == 65535  # 96 bytes per stack: the grid's limit, not the budget's


def test_ranges_the_gpu_suites_build_their_split_cases_on(ask, pkg):
    """the expressions of test_gpu_ssim.py, test_gpu_ssim_rgb.py and test_gpu_distortion_rgb.py"""
    assert (pkg.DCT3D_SSIM_BLOCK_BUDGET, pkg.DCT3D_RGB_PLANE_BUDGET) == (SSIM_BUDGET, PLANE_BUDGET)
    qs, want = [], []
    for D in DEPTHS:
        per_stack = D * (256 // 4) * (176 // 4) * (8 * 32 + 4)  # test_gpu_ssim._range_stacks
        qs.append(("ssimrange", SSIM_BUDGET, 256, 176, D, 32, 1, SSIM_BUDGET // per_stack + 1))
        want.append([per_stack, SSIM_BUDGET // per_stack])
        w, h, stacks = (128, 176, 5) if D == 4 else (128, 88, 5)  # test_gpu_ssim_rgb._range_shape
        rec = D * ((w + 3) // 4) * ((h + 3) // 4) * (8 * 32 + 4) * 3
        qs.append(("ssimrange", SSIM_BUDGET, w, h, D, 32, 3, stacks))
        want.append([rec, SSIM_BUDGET // rec])
        assert SSIM_BUDGET // rec == 3
        for cw, ch in ((256, 176), pkg.chroma_size(256, 176)):  # test_gpu_distortion_rgb.test_stack_ranges
            planes = 32 * D * (256 * 176 + 2 * cw * ch)
            qs.append(("range", PLANE_BUDGET, planes, PLANE_BUDGET // planes + 1, 0))
            want.append([PLANE_BUDGET // planes])
    # the host-pointer staging chunk: test_gpu_ssim_rgb.test_host_call_in_two_chunks, and the guards
    qs += [("range", CHUNK, 1920 * 1080 * 3 * 4, 3, 0), ("range", CHUNK, 0, 5, 0), ("range", CHUNK, 17 * 9 * 8, 0, 0),
           ("range", CHUNK, CHUNK + 1, 4, 0), ("range", CHUNK, CHUNK, 4, 0), ("range", CHUNK, CHUNK // 2, 4, 0), ("range", CHUNK, 8, 3, 0)]
    want += [[2], [1], [1], [1], [1], [2], [3]]
    assert ask(qs) == want


def first_use(idx, n_tables, all_tables):
    used = list(range(n_tables)) if all_tables else list(dict.fromkeys(idx))
    return [len(used)] + used + [used.index(t) if t in used else -1 for t in range(n_tables)]


@pytest.mark.parametrize("cand,n_tables", [([(0, 0, 0)], 1), ([(2, 1, 2), (2, 1, 0), (2, 3, 2), (0, 1, 2)], 4),
                                           ([(3, 1, 2), (1, 2, 3), (8, 8, 8)], 9), ([(i, (i + 5) % 32, (i + 11) % 32) for i in range(32)], 32)])
def test_compaction(ask, cand, n_tables):
    flat = [t for c in cand for t in c]
    qs, want = [], []
    for all_tables in (0, 1):
        qs.append(("compact", 1, n_tables, all_tables, len(flat)) + tuple(flat))  # joint
        want.append(first_use(flat, n_tables, all_tables))
        for k in range(3):  # plane k: every third index from k on
            qs.append(("compact", 3, n_tables, all_tables, len(cand)) + tuple(flat[k:] + flat[:k]))
            want.append(first_use(flat[k::3], n_tables, all_tables))
    assert ask(qs) == want


def sections(sizes):
    out, at = [], 0
    for n in sizes:
        out += [at, n]
        at += n
    return out + [at]


def test_sums_sections_and_index_maps(ask):
    qs, want = [], []
    for n_tables, n_stacks, channels in itertools.product(COUNTS, (1, 2, 5), (1, 3)):
        runs = n_tables * n_stacks * channels
        for f in itertools.product((0, 1), repeat=3):
            qs.append(("sums", runs) + f)
            want.append(sections([runs * v for v in f]))
        ts = n_tables * n_stacks
        qs.append(("c420", ts))
        want.append(sections([3 * ts, ts, ts]) + [v for i in range(ts) for v in (3 * i, 3 * ts + i, 4 * ts + i)])
    for nk, n_stacks, n_cand, bits, n_sp, per in [((1, 1, 1), 1, 1, 0, 0, 1), ((9, 9, 9), 5, 8, 1, 4, 2), ((3, 1, 2), 7, 32, 0, 3, 3),
                                                  ((32, 32, 32), 4, 32, 1, 3, 4), ((2, 8, 1), 3, 9, 1, 0, 5)]:
        nt, n_rgb = sum(nk), n_cand * n_stacks
        # a range's plane sums lie one after another: per range, per plane, [slot][stack of the range]
        where, at = {}, 0
        for s0 in range(0, n_stacks, per):
            for k in range(3):
                for t in range(nk[k]):
                    for s in range(s0, min(s0 + per, n_stacks)):
                        where[k, t, s] = at
                        at += 1
        qs.append(("rgb",) + nk + (n_stacks, n_cand, bits, n_sp, per))
        want.append(sections([nt * n_stacks, nt * n_stacks * bits, n_rgb, 3 * n_rgb * (n_sp >= 3), n_rgb * (n_sp == 4)]) +
                    [nt, 0, nk[0], nk[0] + nk[1]] + [where[k, t, s] for k in range(3) for t in range(nk[k]) for s in range(n_stacks)])
    for n_stacks, channels, s0, ch, unit in [(1, 1, 0, 0, 1), (5, 3, 2, 1, 1), (5, 3, 2, 2, 8 * 479 * 269), (7, 1, 6, 0, 1)]:
        qs += [("place", 0, n_stacks, channels, s0, ch, unit), ("place", 1, n_stacks, channels, s0, ch, unit)]
        want += [[(s0 * channels + ch) * unit, n_stacks * channels * unit, channels * unit],
                 [(ch * n_stacks + s0) * unit, channels * n_stacks * unit, unit]]
    for o, n_stacks, s0, ns, inner in [(0, 1, 0, 1, 1), (3, 7, 4, 2, 3), (31, 5, 4, 1, 1)]:
        qs.append(("chunk", o, n_stacks, s0, ns, inner))
        want.append([o * ns * inner, (o * n_stacks + s0) * inner, (o * n_stacks + s0) * 3 + 2])
    assert ask(qs) == want

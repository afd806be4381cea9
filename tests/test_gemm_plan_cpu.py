"""The GEMM launcher's plan (csrc/gemm_plan.h: kernel family, ring tile, skinny split-K and row passes, gemm_rows tile; no HIP) printed by
the stand-alone host program tests/host/gemm_plan_main.cpp, compiled with -fsanitize=address,undefined and run directly, against
tests/golden/gemm_plan.txt.  That file was recorded from the decision lines of the launcher BEFORE the plan existed (the commit that
introduced gemm_plan.h says how), so a difference is a shape that a change moved onto another kernel: the assertion names the lines."""
import os
import shutil
import subprocess

import pytest

import gemm_plan_golden as gpg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_of_every_recorded_shape_under_host_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "gemm_plan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "gemm_plan_main.cpp"), "-o", str(exe)], check=True, timeout=300)
    run = subprocess.run([str(exe), gpg.GOLDEN, "20"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stderr.strip())       # plans per second: information only
    want = gpg.lines()
    got = run.stdout.splitlines()
    moved = [f"{w}   NOW: {g.partition(' -> ')[2]}" for w, g in zip(want, got) if w != g]
    assert not moved, "\n".join([f"{len(moved)} shapes moved:"] + moved[:40])
    assert len(got) == len(want)
    assert sum(" ->" in w for w in want) > 300


def test_recorded_rule_matches_the_table_of_its_thresholds():
    """(m, n, K) -> tile, each threshold of the ring rule from both sides, derived by hand from the launcher's code; the tiles that forced
    switches degrade to on narrow outputs; the block-maximum override."""
    table = [((5504, 1536, 256), "128x64"), ((5504, 256, 1024), "64x64"), ((32768, 1024, 256), "128x128"), ((5000, 4097, 1024), "128x128"),
             ((3800, 3000, 2048), "256x256-8phase"), ((3584, 3000, 2048), "128x128"), ((3584, 4096, 1024), "256x256-8phase"),
             ((3328, 4096, 1024), "128x128"), ((8192, 512, 1024), "128x128"), ((8064, 512, 1024), "128x64"), ((1280, 1024, 64), "128x64"),
             ((1152, 1024, 64), "64x64"), ((2561, 4096, 2048), "256x256-8phase"), ((2560, 4096, 2048), "128x128")]
    for (m, n, k), tile in table:
        assert gpg.ring_tile(m, n, k) == tile, (m, n, k)
    assert gpg.ring_tile(64, 33, 256, mode=1) == "128x64"
    assert gpg.ring_tile(64, 33, 256, mode=4) == "64x64" and gpg.ring_tile(64, 33, 256, mode=5) == "64x64"
    assert gpg.ring_tile(64, 100, 6144, blockmax=True) == "128x128" and gpg.ring_tile(64, 100, 6144, mode=3, blockmax=True) == "128x128"


def test_recorded_file_holds_every_required_shape():
    """The recorded file is also the program's shape list, so a deleted line would shrink what the comparison covers: the shapes it must
    hold are listed here independently of it -- the GPU tests' own lists, the convolution tile table (whose recorded kernel is the one
    the table expects), the shapes the rule's comments name, the skinny grid, and a skinny shape the launcher rejects."""
    import conv_tile_cases as ctc
    import test_bench_shapes_gpu as tb

    have = {ln.partition(" ->")[0]: ln.partition(" ->")[2].strip() for ln in gpg.lines() if " ->" in ln}

    def ring(m, n, k, bm=0):
        plan = have.get(f"ring m={m} n={n} k={k} bm={bm}")
        assert plan is not None, (m, n, k, bm)
        assert [tok.split(":")[0] for tok in plan.split()] == ["-1", "0", "1", "2", "3", "4", "5"], plan      # every forced switch

    for m, k, n in [s[:3] for s in tb.RING_SHAPES] + tb.EIGHT_PHASE_SHAPES:
        ring(m, n, k)
    for (m, n, k), _ in tb.RULE_BRANCH_SHAPES:
        ring(m, n, k)
    for m, n, k in [(15360, 3072, 5120), (15360, 8192, 3072), (23680, 1024, 4096), (8192, 8192, 8192), (44032, 1536, 256)]:
        ring(m, n, k)
    ring(256, 100000, 6144)
    ring(256, 100000, 6144, bm=1)
    for c in ctc.CASES + ctc.EPILOGUE_SHAPES + ctc.VIEW_SHAPES:
        m, n, taps, _, plain = ctc.geometry(c)
        key = (f"gemm m={m} n={n} cin={c['cin']} cin_pad={(c['cin'] + 63) // 64 * 64} taps={taps} plain={int(plain)} x16={int(c['x16'])} "
               f"o16={int(c['out16'])} al=1 bm=0 ga=0 ln=0 ws=0 ring=-1 nosplit=0")
        assert have.get(key) == c["expected"], (c["id"], have.get(key))
    for m in (1, 16, 17, 32):
        for kp in (64, 1024, 1088, 2048, 4096):
            for n in (256, 1024, 2048, 2064):
                plan = have.get(f"skinny m={m} n={n} kp={kp}")
                assert plan is not None and len(plan.split()[0]) == 16, (m, n, kp, plan)       # all 16 combinations of the extras
    assert any(k.startswith("skinny ") and "skinny invalid" in v for k, v in have.items())
    assert sum(k.startswith("rows ") for k in have) >= 90

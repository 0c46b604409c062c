"""The piece-table splitter of the sharded merge's finish (csrc/merge_pieces.h), host side.  The GPU suites reach
it only through whole merges (tests/test_aligner_gpu.py, tests/test_uncertainty_gpu.py); here it runs alone."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_pieces_header_under_sanitizers(tmp_path):
    """csrc/merge_pieces.h (plain C++; both finish entry points of csrc/merge.hip launch once per range it
    yields) in a stand-alone program built with AddressSanitizer + UBSan, sanitizer runtimes linked statically,
    with 1 and with 2 doubles per pixel:

    - 70 one-frame pieces over 70 frames, HW = 2^28: every offset is i · k · HW.  A table holds MAXPIECES = 64
      entries, so the window is cut after its 64th frame: two ranges of 64 and 6 pieces, not one;
    - 70 pieces that each span all of a 4-frame window: refused, naming frame f0 and the count 70;
    - a per-frame count that reaches 64 and never exceeds it (3 pieces over the whole 40-frame window, 61
      one-frame pieces on frame 10, one on each later frame): the ranges partition the window, each is as long
      as its table allows and lists ≤ 64 pieces in their original order, each at the offset of all earlier
      pieces, in range or not;
    - zero-length pieces: never listed (70 of them on one frame are an empty table, no refusal), yet the
      offsets count them, by 0;
    - nf = 0 (no range) and npieces = 0 (one range, empty table)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/cpp/merge_pieces_check.cpp"
    exe = str(tmp_path / "merge_pieces_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "rollingdepth_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "merge_pieces_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout and "16 cases" in r.stdout, r.stdout

"""Host: the address rule of the row pass's warm-up (spmf_amd/csrc/row_prefetch.h row_warm_word).

The kernel reads, by scalar loads, one entry word of every 64-byte half of every 128-byte line that the first
min(n, 128) words of a coming row span.  tools/row_prefetch_host.cpp is a stand-alone program (its own main) that
includes the very header the kernel includes, enumerates n = 0 ... 300 and all 32 alignments of the row's start inside
a line, and fails if an index lies outside [0, n), or a spanned 128-byte line, or a spanned unit of the ladder's step,
is not touched.  It is built here with -fsanitize=address,undefined and run on the CPU, with the step the library is
built with (16 words) and with the variant of one load per line (-DROW_PREFETCH_WORDS=32)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("words", [16, 32])
def test_every_index_is_a_word_of_the_row_and_every_line_is_touched(tmp_path, words):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / f"row_prefetch_host_{words}")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-DROW_PREFETCH_WORDS={words}",
                            "-I", os.path.join(ROOT, "spmf_amd", "csrc"),
                            os.path.join(ROOT, "tools", "row_prefetch_host.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert run.stdout.startswith(f"ok: {301 * 32} (n, alignment) cases") and f"{words} words apart" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]


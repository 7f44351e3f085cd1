"""Host sanitizer run of the error cells of the dense edge stream: `make -C
csrc build/fuzz/errcell_check` builds csrc/fuzz/errcell_check.cpp with
-fsanitize=address,undefined.  Over random layouts of the small carve the
program holds pack_word_entry to an independent restatement, error *
2^cell_bits + cell below 2^cell_bits + cells, for every word with a cell of the
layout, and an exact model of the kernel's span path and flush — two entries
per cell, the error count read off the error entries — to a direct computation
of count, errors, sum, min, max and histogram.  No GPU."""
import os
import subprocess

from conftest import PKG_DIR

CSRC = PKG_DIR / "csrc"


def test_error_cells_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "build/fuzz/errcell_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(CSRC / "build" / "fuzz" / "errcell_check")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) > 1_000_000

"""Host sanitizer run of the span-word formats (csrc/span_word.h): `make -C
csrc wordcheck` builds csrc/fuzz/span_word_check.cpp with
-fsanitize=address,undefined.  The program packs and unpacks cell words at
every bin exponent 0..26 and at the borders of the bins (lo, hi, lo +- 1), under
residual widths below, at and above the exponent and ranges that hold the bin
or not: a word either round-trips to (code, error, duration) or carries the
escape value, exactly when the rule restated in the program says so; keys
order as durations within a code; and the all-ones word is a skip word under
every width combination, one code and one cell included.  No GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR

CSRC = PKG_DIR / "csrc"


@pytest.fixture(scope="module")
def checker():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "wordcheck"], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr and "asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    return CSRC / "build" / "fuzz" / "span_word_check"


def test_cell_words_under_asan_ubsan(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(checker)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) > 1_000_000

"""Host sanitizer run of the packed-word format (csrc/span_word.h): `make -C
csrc packcheck` builds csrc/fuzz/pack_word_check.cpp with
-fsanitize=address,undefined and runs it.  The program holds pack and unpack to
an independent restatement of the rule over random layouts (which layouts
pack, the residual width, which spans escape and which of them are wide), and
checks the field extremes, the reserved values under every width, key order
against duration order within a code, the code an escape word carries, and the
split into the column's two planes with its rejoin.  No GPU."""
import os
import subprocess

from conftest import PKG_DIR

CSRC = PKG_DIR / "csrc"


def test_packed_words_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", str(CSRC), "build/fuzz/pack_word_check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(CSRC / "build" / "fuzz" / "pack_word_check")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    word, checks = r.stdout.split()
    assert word == "ok" and int(checks) > 1_000_000

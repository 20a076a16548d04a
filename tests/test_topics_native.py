"""The topic records' parse and flatten under AddressSanitizer + UBSan.

``csrc/core/topic_follower.cpp`` reads values that anybody can put under the topics prefix
of the store.  Its pure part (``topic_parse_record``, ``topic_parse_key``,
``topics_flatten``) is linked into a host program of its own
(tests/native/topics_parse.cpp) -- the sanitizer runtime has to own the process, nothing is
preloaded -- and run over a hostile corpus and a few thousand generated records.  Any
sanitizer report fails the test.
"""
import os
import subprocess

from ptype_amd import _build

REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_topics_parse_under_address_sanitizer():
    exe = _build.build_native_test("address", program="topics_parse")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    found = [x for x in REPORTS if x in out]
    assert not found, f"address sanitizer reports {found}:\n{out[-6000:]}"
    assert r.returncode == 0, out[-4000:]
    for s in ("hostile", "generated", "topics_parse"):
        assert f"OK {s}" in r.stdout

"""The topic records' ``queue`` field under AddressSanitizer + UBSan.

``topic_parse_record`` reads ``queue`` from values that anybody can put under the topics
prefix of the store, and ``topics_flatten`` lays the queue subscriptions out behind the
ordinary ones.  Both are linked into a host program of its own
(tests/native/queues_parse.cpp) -- the sanitizer runtime has to own the process, nothing is
preloaded -- and run over a hostile corpus for the field and a few thousand generated mixed
record sets; the program checks that the ordinary arrays are those of the records without
the queue records, and the queue arrays' consistency.  Any sanitizer report fails the test.
"""
import os
import subprocess

from ptype_amd import _build

REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_queues_parse_under_address_sanitizer():
    exe = _build.build_native_test("address", program="queues_parse")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=240)
    out = r.stdout + r.stderr
    found = [x for x in REPORTS if x in out]
    assert not found, f"address sanitizer reports {found}:\n{out[-6000:]}"
    assert r.returncode == 0, out[-4000:]
    for s in ("hostile", "generated", "queues_parse"):
        assert f"OK {s}" in r.stdout

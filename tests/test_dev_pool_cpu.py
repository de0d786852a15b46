"""The caching pool of device blocks (csrc/dev_pool.h) on the host: tests/hostcheck/pool_check.cpp drives its bookkeeping against
a policy that counts mallocs, frees, queued stream waits and host waits and whose events pass when the case says so.  Built with
the address and undefined-behaviour sanitizers, like the other host checks; no GPU and no HIP header is involved."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostcheck", "pool_check.cpp")

CASES = ["same_stream",      # a block tagged with the asking stream: no wait, no malloc
         "cross_stream",     # another stream: exactly one queued wait on the batch's event, none once it has passed
         "streamless",       # get(dev, n): untagged first, then passed events, then a host wait; malloc only for an empty class
         "release_all",      # waits for every pending event, then frees everything; also on an allocation failure
         "seal",             # one event, recorded at the sealing put, for every batch of the stream that had none; none afterwards
         "events_bounded",  # 1 000 put/get rounds: events go back to the cache with the last block of their batch
         "classes",          # the size classes, against values worked out by hand
         "ignored_puts"]     # null, unknown and repeated puts


@pytest.fixture(scope="module")
def pool_check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool_hostcheck") / "pool_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "fre-nctools_amd", "csrc"), SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("case", CASES)
def test_pool(pool_check_exe, case):
    r = subprocess.run([pool_check_exe, case], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok " + case), r.stdout

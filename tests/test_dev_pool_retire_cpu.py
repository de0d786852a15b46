"""DevPool::retire (csrc/dev_pool.h) on the host: tests/hostcheck/pool_retire_check.cpp drives it against a policy that knows which
stream every event was recorded on.  After retire(stream) the pool holds no event of that stream, sealed or still to be recorded,
never asks about one, hands the stream's blocks out as untagged ones, and leaves other streams' batches as they were.  Built with
the address and undefined-behaviour sanitizers, like tests/test_dev_pool_cpu.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_retire(tmp_path):
    exe = str(tmp_path / "pool_retire_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "fre-nctools_amd", "csrc"), os.path.join(HERE, "hostcheck", "pool_retire_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout

"""The policy of the forward pass's graph cache on the CPU: csrc/graph_cache.h driven by tests/cpu/graph_cache_test.cpp (built with
g++, an integer in the executable's place) -- key equality over all five fields, first-in-first-out eviction at the capacity, one
`retire` per executable, the `uses` counter of a re-inserted key, and the documented thrashing past 64 keys.  What `retire` waits for
on the device is tests/test_gpu_device_api.py's business."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_cache_policy(tmp_path):
    exe = tmp_path / "graph_cache_test"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpu", "graph_cache_test.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
    assert r.stdout.decode().strip() == "graph_cache_test: all checks passed"

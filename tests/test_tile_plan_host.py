"""The tile kernels' plan (aither_amd/csrc/agx_tile_plan.hpp) checked on the host.

tests/cpp/tile_plan.cpp includes the header the kernels decode their ranges with and walks
every range of both orders: coverage, segments, the column order's equal cut, the cost bound
and, at 256^3, how many neighbouring columns the step order brings together.  Built here
with the address and undefined-behaviour sanitizers.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tile_plan(tmp_path):
    exe = str(tmp_path / "tile_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(HERE, "cpp", "tile_plan.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, out
    assert "tile plan OK" in out

"""The patch plan of the matrix residual (aither_amd/csrc/agx_mresid_plan.hpp), host side: one
k-step of k_matrix_resid_d2m replayed under the address and undefined-behaviour sanitizers
(tests/cpp/mresid_plan.cpp), and the places that have to name the header."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_plan_under_the_sanitizers():
    subprocess.run(["make", "-C", CPP, "-f", "mresid.mk"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(CPP, "mresid_plan")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"mresid_plan: (\d+) planes, (\d+) patches walked", run.stdout)
    # (the benchmark's 262 x 262 plane alone needs 262 * 262 / 256 = 269 patches of 256 threads)
    assert m and int(m.group(1)) >= 15 and int(m.group(2)) > 269, run.stdout


def test_host_and_kernel_share_the_one_plan():
    assert "agx_mresid_plan.hpp" in _read("aither_amd", "csrc", "Makefile")
    assert '#include "agx_mresid_plan.hpp"' in _read("aither_amd", "csrc", "agx_lusgs.hpp")
    plan = _read("aither_amd", "csrc", "agx_mresid_plan.hpp")
    assert "hip" not in plan.lower().replace("__hipcc__", "")       # plain C++
    kernel = _read("aither_amd", "csrc", "agx_lusgs_kernels.hpp")
    api = _read("aither_amd", "csrc", "agx_api.hip")
    for call in ("mrp_deal(", "mrp_patch(", "mrp_own(", "mrp_extra(", "mrp_neighbour("):
        assert call in kernel, call
    assert "mrp_wgs(" in api and "mrp_per_xcd(" in api
    # the position chunks of the earlier marching form are gone from its launch
    assert "MR_WAVES" not in kernel and "MR_WAVES" not in api

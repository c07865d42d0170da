"""The flux, limiter and boundary branches that only the FLOW selects, HIP vs CPU oracle.

Every other synthetic parity deck starts from synthetic.perturbed_state: Mach 0.16, three
positive velocity components -- one side of every data-dependent branch of ausm_flux,
roe_flux, ghost_state, extrap_hold and of the implicit off-diagonals.  Here the decks of
tests/flow_cases.py run on the transonic, sign-changing field of tests/flow_fields.py;
tests/test_flow_branches_host.py proves on the oracle (tests/branch_census.py) that each
claimed arm is taken by >= 8 faces before every compared step and that no boundary face sits
on a threshold.

a. parity: parity_utils.run_pair unchanged (RTOL 1e-10, the derived matrix-residual bound,
   state / residual / dt), three steps per case, all four libraries;
b. kernel forms: the production tile kernels against their march / gather forms and the k-plane
   LU-SGS sweep against the hyperplane one at 1e-12, as the tests of the same names in
   tests/test_parity_gpu.py -- the fused and tiled kernels have separate code per direction
   and side, and a transonic field is where a wrong side shows.
"""
import numpy as np
import pytest

import aither_amd
import flow_cases
from parity_utils import rel_err, run_pair
from test_parity_gpu import _run_with_env

pytestmark = pytest.mark.gpu

CP, TP = "caloricallyPerfect", "thermallyPerfect"


def _lib(spec):
    return aither_amd.load(spec["lib"], TP if spec["tp"] else CP)


@pytest.mark.parametrize("name", sorted(flow_cases.CASES))
def test_transonic_parity(oracle, name):
    spec = flow_cases.CASES[name]
    case = flow_cases.build(spec)
    if spec["tp"]:
        import tp_cases
        tp_cases.excited(case)
    sg, so = run_pair(_lib(spec), oracle, case, spec["steps"])
    if spec["lib"] == 7:
        # k and omega are orders of magnitude away from the flow variables: every component
        # against its OWN scale as well (as test_rae2822_rans_parity)
        g = case.ng
        a = sg.download("state", 0)[g:-g, g:-g, g:-g]
        b = so.download("state", 0)[g:-g, g:-g, g:-g]
        for e in range(7):
            scale = np.abs(b[..., e]).max() or 1.0
            assert np.abs(a[..., e] - b[..., e]).max() <= 1e-10 * scale, e
    sg.close(), so.close()


def _forms(agx, name, var, kinds):
    spec = flow_cases.FORMS[name]
    case = flow_cases.build(spec)
    ref = _run_with_env(agx, case, spec["steps"], {var: kinds[0]})
    assert np.all(np.isfinite(ref))
    for kind in kinds[1:]:
        got = _run_with_env(agx, case, spec["steps"], {var: kind})
        assert rel_err(got, ref) < 1e-12, kind


def test_kernel_variants_agree(agx):
    """tile / march / gather on AUSM + WENO, (70, 13, 9), the stream against i"""
    _forms(agx, "kernel", "AGX_KERNEL", ("tile", "march", "gather"))


def test_viscous_kernel_forms_agree(agx):
    """LDS-staged / face-once / one-thread-per-cell viscous residual, (70, 15, 9), a viscous
    wall beside the stream"""
    _forms(agx, "visc", "AGX_VISC", ("tile", "march", "gather"))


def test_lusgs_sweep_forms_agree(agx):
    """k-plane pipeline against a launch per hyperplane, two sweeps, viscous AUSM"""
    _forms(agx, "lusgs", "AGX_LUSGS", ("kp", "plane"))

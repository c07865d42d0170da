"""Thermally perfect gas, host side (no GPU): the fixture of the reference's thermallyPerfect
case, the case build, the numpy restatement of the model (aither_amd.case.fluid) and the two
thermally perfect libraries (load and exports only)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aither_amd
from aither_amd import abi
from aither_amd.case import fluid, synthetic
from aither_amd.case.builder import build_case, config_struct
from aither_amd.case.inputfile import parse_input

HERE = os.path.dirname(os.path.abspath(__file__))
TP_DIR = os.path.join(HERE, "golden", "thermallyPerfect")
TP_INP = os.path.join(TP_DIR, "thermallyPerfect.inp")
CASES = os.path.join(HERE, "golden", "cases")
TRUTH = [5.8177e-01, 3.8066e-01, 4.8670e-01, 1.0000e+00, 5.9931e-01, 1.2830e-06, 3.5031e-04]


def test_fixture_digests_and_truth_record():
    spec = json.load(open(os.path.join(TP_DIR, "truth.json")))
    assert spec["truth"] == TRUTH
    assert spec["iterations"] == 20 and spec["ignore"] == [3] and spec["line"] == 468
    for f in ("thermallyPerfect.inp", "thermallyPerfect.xyz"):
        data = open(os.path.join(TP_DIR, f), "rb").read()
        assert hashlib.sha256(data).hexdigest() == spec["sha256"][f], f
    out = subprocess.check_output([sys.executable, os.path.join(TP_DIR, "make_fixture.py"),
                                   "--manifest"], text=True)
    assert "matches truth.json" in out


def test_truth_deck_builds_thermally_perfect():
    case = build_case(TP_INP)
    assert case.n_eq == 7 and case.ng == 1 and len(case.blocks) == 1
    assert tuple(case.blocks[0].geom.n) == (120, 150, 1)
    cfg = config_struct(case)
    assert cfg.thermodynamic_model == abi.THERMO["thermallyPerfect"] == 1
    assert cfg.gas.n_vib == 1 and cfg.gas.theta_v[0] == 3056.0 / 2000.0
    assert list(cfg.gas.theta_v[1:]) == [0.0] * (abi.MAX_VIB - 1)
    # a_ref and R stay the calorically perfect ones (input.cpp:608-613)
    cpg = fluid.make_gas("air", 2000.0, 0.4, 1.0)
    assert cfg.gas.a_ref == cpg.a_ref and cfg.gas.gas_constant == cpg.gas_constant


@pytest.mark.parametrize("name", sorted(os.listdir(CASES)))
def test_existing_decks_stay_calorically_perfect(name):
    path = os.path.join(CASES, name, name + ".inp")
    deck = parse_input(path)
    deck.multigrid_levels = 1       # (the finest level; the gas does not depend on it)
    cfg = config_struct(build_case(path, deck=deck))
    assert cfg.thermodynamic_model == 0 and cfg.gas.n_vib == 0
    assert list(cfg.gas.theta_v) == [0.0] * abi.MAX_VIB


def test_validate_accepts_thermally_perfect_by_name_only():
    deck = synthetic.make_deck(thermodynamic_model="thermallyPerfect")
    deck.validate()
    deck.thermodynamic_model = "frozenChemistry"
    with pytest.raises(NotImplementedError, match="thermodynamicModel frozenChemistry"):
        deck.validate()


@pytest.fixture
def air():
    return fluid.make_gas("air", 2000.0, 0.4, 1.0, "thermallyPerfect")


def test_cv_limits(air):
    r, n = air.gas_constant, air.n
    # T -> 0: the vibrational mode is frozen; T -> infinity: fully excited (+R)
    assert abs(fluid.cv(air, 1.0e-3) / (n * r) - 1.0) < 1e-14
    assert abs(fluid.cv(air, 1.0e5) / ((n + 1.0) * r) - 1.0) < 1e-9
    t = np.geomspace(1.0e-3, 1.0e5, 400)
    c = fluid.cv(air, t)
    assert np.all(c >= n * r) and np.all(c <= (n + 1.0) * r)
    np.testing.assert_allclose(fluid.cp(air, t), c + r, rtol=1e-15)
    np.testing.assert_allclose(fluid.gamma(air, t), (c + r) / c, rtol=1e-15)
    # without vibrational modes: the calorically perfect constants
    cpg = fluid.make_gas("air", 2000.0, 0.4, 1.0)
    assert np.all(fluid.cv(cpg, t) == n * r)


def test_energy_derivative_is_cv(air):
    t = np.geomspace(0.01, 50.0, 200)
    h = 1.0e-5 * t
    de = (fluid.spec_energy(air, t + h) - fluid.spec_energy(air, t - h)) / (2.0 * h)
    np.testing.assert_allclose(de, fluid.cv(air, t), rtol=1e-8)


def test_temperature_from_energy_inverts_spec_energy(air):
    t = np.geomspace(0.01, 50.0, 2001)
    got = fluid.temperature_from_energy(air, fluid.spec_energy(air, t))
    np.testing.assert_allclose(got, t, rtol=1e-13, atol=0.0)


def test_tp_libraries_export_exactly_the_c_abi():
    for path in (aither_amd.TP_LIB_PATH, aither_amd.RANS_TP_LIB_PATH):
        assert os.path.exists(path), "not built: run __graft_entry__.build()"
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        names = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
        assert names and all(n.startswith("agx_") for n in names)
        assert {n[4:] for n in names} == set(abi.SYMBOLS)


def test_all_four_libraries_load_global_in_one_process():
    code = ("import ctypes, sys\n"
            "libs = [ctypes.CDLL(p, mode=ctypes.RTLD_GLOBAL) for p in sys.argv[1:]]\n"
            "for l in libs:\n"
            "    l.agx_version.restype = ctypes.c_char_p\n"
            "print('|'.join(l.agx_version().decode() for l in libs))\n")
    paths = [aither_amd.LIB_PATH, aither_amd.RANS_LIB_PATH, aither_amd.TP_LIB_PATH,
             aither_amd.RANS_TP_LIB_PATH]
    out = subprocess.check_output([sys.executable, "-c", code, *paths], text=True)
    versions = out.strip().split("|")
    assert len(versions) == 4 and all("gfx950" in v for v in versions)
    assert ["thermallyPerfect" in v for v in versions] == [False, False, True, True]


def test_loader_picks_the_library_of_the_model():
    assert aither_amd.lib_path(5) == aither_amd.LIB_PATH
    assert aither_amd.lib_path(7) == aither_amd.RANS_LIB_PATH
    assert aither_amd.lib_path(5, "thermallyPerfect") == aither_amd.TP_LIB_PATH
    assert aither_amd.lib_path(7, "thermallyPerfect") == aither_amd.RANS_TP_LIB_PATH
    with pytest.raises(ValueError, match="thermodynamic_model"):
        aither_amd.load(5, "thermallyImperfect")
    with pytest.raises(ValueError, match="n_eq"):
        aither_amd.lib_path(6, "thermallyPerfect")
    api = aither_amd.load(7, "thermallyPerfect")
    assert b"thermallyPerfect" in api.version()
    assert aither_amd.load(7, "thermallyPerfect") is api and aither_amd.load(7) is not api
    # the environment overrides, as for the other two libraries
    code = "import aither_amd; print(aither_amd.lib_path(5, 'thermallyPerfect'))"
    env = dict(os.environ, AGX_TP_LIB="/elsewhere/libtp.so")
    out = subprocess.check_output([sys.executable, "-c", code], text=True, env=env,
                                  cwd=os.path.dirname(HERE))
    assert out.strip() == "/elsewhere/libtp.so"

"""Loader for the in-tree HIP library (fails loudly; there is no fallback)."""
import ctypes
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# AGX_LIB: a diagnostic build of the same library (e.g. -DAGX_KP_TRACE)
LIB_PATH = os.environ.get("AGX_LIB") or os.path.join(_HERE, "libaither_gfx950.so")
# the same sources built for the 7-equation set (rans: + k, omega), same C-ABI
RANS_LIB_PATH = os.environ.get("AGX_RANS_LIB") or os.path.join(_HERE, "libaither_gfx950_rans.so")
# both again for the thermally perfect gas (-DAGX_TPG=1), same C-ABI
TP_LIB_PATH = os.environ.get("AGX_TP_LIB") or os.path.join(_HERE, "libaither_gfx950_tp.so")
RANS_TP_LIB_PATH = (os.environ.get("AGX_RANS_TP_LIB") or
                    os.path.join(_HERE, "libaither_gfx950_rans_tp.so"))
THERMODYNAMIC_MODELS = ("caloricallyPerfect", "thermallyPerfect")
_api = {}


def lib_path(n_eq=5, thermodynamic_model="caloricallyPerfect"):
    """Path of the library that serves `n_eq` equations (5: euler / navierStokes, 7: rans)
    with `thermodynamic_model` (caloricallyPerfect / thermallyPerfect)."""
    if n_eq not in (5, 7):
        raise ValueError("n_eq is 5 or 7")
    if thermodynamic_model not in THERMODYNAMIC_MODELS:
        raise ValueError(f"thermodynamic_model {thermodynamic_model!r} is not one of "
                         f"{', '.join(THERMODYNAMIC_MODELS)}")
    tp = thermodynamic_model == "thermallyPerfect"
    if n_eq == 5:
        return TP_LIB_PATH if tp else LIB_PATH
    return RANS_TP_LIB_PATH if tp else RANS_LIB_PATH


def load(n_eq=5, thermodynamic_model="caloricallyPerfect"):
    """Return the bound C-ABI of libaither_gfx950.so (n_eq = 5: euler /
    navierStokes) or libaither_gfx950_rans.so (n_eq = 7: rans), or of their thermally
    perfect builds libaither_gfx950_tp.so / libaither_gfx950_rans_tp.so."""
    path = lib_path(n_eq, thermodynamic_model)
    key = (n_eq, thermodynamic_model)
    if key not in _api:
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _api[key] = abi.Api(ctypes.CDLL(path), "agx_")
    return _api[key]

"""The id ranges of agx_output_pack and the field ranges of agx_field_upload /
agx_field_download (aither_amd/csrc/agx_out_ranges.hpp), host side: the table's classifier held,
text for text, to the cascade it replaced under the address and undefined-behaviour sanitizers
(tests/cpp/out_ranges.cpp), and the places that have to name the header."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_the_table_is_the_cascade_under_the_sanitizers():
    subprocess.run(["make", "-C", CPP, "-f", "out_ranges.mk"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(CPP, "out_ranges")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"out_ranges: (\d+) lists compared", run.stdout)
    # (37 boundary ids: 37 + 37^2 + 37^3 lists of them, and 9 * 57 of one id repeated)
    assert m and int(m.group(1)) >= 50000, run.stdout


def test_the_entry_points_share_the_one_table():
    assert "agx_out_ranges.hpp" in _read("aither_amd", "csrc", "Makefile")
    api = _read("aither_amd", "csrc", "agx_api.hip")
    assert '#include "agx_out_ranges.hpp"' in api
    table = _read("aither_amd", "csrc", "agx_out_ranges.hpp")
    assert "hip" not in table.lower()                               # plain C++
    for call in ("out_classify(", "field_is_stats(", "field_is_series(", "field_is_spectra("):
        assert call in api, call
    # each range is stated in the table and nowhere in the entry points
    assert "AGX_CSTAT_END" in table and "AGX_CSTAT_END" not in api
    assert "AGX_FLUX_END" in table and "AGX_FLUX_END" not in api

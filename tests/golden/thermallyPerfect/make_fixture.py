#!/usr/bin/env python3
"""How tests/golden/thermallyPerfect/ is made (the default and --write need the reference).

The reference's thermallyPerfect regression case (rans SST 2003 on a supersonic ramp, air
as a thermally perfect gas) is kept apart from tests/golden/cases/: the CPU oracle has no
thermally perfect gas, so the case is not one of the truth vectors it is run over
(regression_truths.json).  This script

  * copies the case's two DATA files, thermallyPerfect.inp and thermallyPerfect.xyz, byte
    for byte -- nothing of the reference's code is copied;
  * transcribes its truth vector, iteration count, ignored column and the line of
    testCases/regressionTests.py the vector stands on into truth.json, with the SHA-256 of
    both data files.

  python make_fixture.py REFERENCE_ROOT            verify this directory against what the
                                                   reference yields (default)
  python make_fixture.py REFERENCE_ROOT --write    (re)generate the data files and truth.json
  python make_fixture.py --manifest                verify the data files against the digests
                                                   in truth.json (no reference needed)
"""
import filecmp
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CASE = "thermallyPerfect"
FILES = (CASE + ".inp", CASE + ".xyz")
sys.path.insert(0, os.path.dirname(HERE))
from make_fixtures import parse_truth  # noqa: E402  (the same transcription as the others)


def sha256(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def generate(ref, dst):
    text = open(os.path.join(ref, "testCases", "regressionTests.py")).read()
    for f in FILES:
        shutil.copy(os.path.join(ref, "testCases", CASE, f), os.path.join(dst, f))
    # both process counts carry the same vector (regressionTests.py:463-470); take the
    # 1-process one, as for the other cases
    truth = parse_truth(text, CASE, 1)
    truth["sha256"] = {f: sha256(os.path.join(dst, f)) for f in FILES}
    return truth


def check_manifest():
    truth = json.load(open(os.path.join(HERE, "truth.json")))
    assert {"truth", "iterations", "ignore", "line", "sha256"} <= set(truth), sorted(truth)
    for f in FILES:
        assert sha256(os.path.join(HERE, f)) == truth["sha256"][f], f
    print(f"tests/golden/{CASE}/ matches truth.json: {len(FILES)} data files, "
          f"{len(truth['truth'])} residuals after {truth['iterations']} iterations")


def main():
    if "--manifest" in sys.argv:
        return check_manifest()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit(__doc__)
    ref = args[0]
    if "--write" in sys.argv:
        truth = generate(ref, HERE)
        with open(os.path.join(HERE, "truth.json"), "w") as fh:
            json.dump(truth, fh, indent=1)
            fh.write("\n")
        print("wrote", ", ".join(FILES), "and truth.json")
        return
    with tempfile.TemporaryDirectory() as tmp:
        truth = generate(ref, tmp)
        _, mismatch, errors = filecmp.cmpfiles(tmp, HERE, list(FILES), shallow=False)
        assert not mismatch and not errors, (mismatch, errors)
    committed = json.load(open(os.path.join(HERE, "truth.json")))
    assert committed == truth, (committed, truth)
    print(f"tests/golden/{CASE}/ reproduced from {ref}")


if __name__ == "__main__":
    main()

"""Every entry point of chase_amd/csrc/capi_gev.hip, fp64 and fp32, launches what the build recorded in
tests/golden/gev_launches.json launched - the same operator-log lines in the same order, nested lines included - and computes the
same bits.  The cases, their shapes and what is hashed: tests/gev_launch_cases.py.  The file was recorded with a build of the
commit before the drivers were written once for both precisions and is never regenerated from the build under test."""
import json
import os

import pytest

import gev_launch_cases as L

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gev_launches.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ran(ctx):
    return L.run_cases(ctx)


def test_every_case_is_recorded_and_run(gold, ran):
    assert list(ran) == list(gold["cases"])
    assert len(ran) == 2 * (20 + 10)             # real and complex: 20 fp64 cases, 10 fp32 cases


def test_oplog_lines_are_those_of_the_recording(gold, ran):
    """never skipped: the lines hold names and shapes only"""
    for name, want in gold["cases"].items():
        got = ran[name]["lines"]
        assert len(got) == len(want["lines"]), (name, len(got), len(want["lines"]))
        for i, (g, w) in enumerate(zip(got, want["lines"])):
            assert g == w, (name, i, g, w)
        assert got[0].split()[0] == name.split()[0]                  # the entry point's own line comes first


def test_output_bits_are_those_of_the_recording(ctx, gold, ran):
    ncu = ctx.info()["num_cu"]
    if ncu != gold["num_cu"]:
        pytest.skip(f"the fp64 GEMM plan depends on the number of compute units: recorded on {gold['num_cu']}, this device has {ncu}")
    moved = [name for name, want in gold["cases"].items() if ran[name]["inputs"] != want["inputs"]]
    bad = [name for name, want in gold["cases"].items() if name not in moved and ran[name]["sha256"] != want["sha256"]]
    assert not bad, bad
    if moved:
        pytest.skip(f"this host's LAPACK gave the seeded generators other input bits than the recording host's in {len(moved)} of "
                    f"{len(ran)} cases, whose output hashes do not apply: {moved}")

"""What the DFT-spread calls of the C ABI refuse, and what they return without doing anything (-m gpu): every public call of
csrc/capi_dft.hip, capi_dft_tx.hip and capi_despread.hip, and the three of capi_mrc.hip that share their argument checks, over the
table of tests/despread_refusal_cases.py in its three states of the handles' allocation sets -- status and the exact
ofdm_last_error() text against tests/golden/despread_refusals.json.  The fixture is recorded from the library of the commit in
front of a change to these files (tests/golden/gen_despread_refusals.py), never from the tree under test: the order in which a
call reports its errors is behaviour, and it differs per call on purpose.  A GPU is needed for the two handles only; no case
launches a kernel."""
import json
import os

import pytest

import despread_refusal_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ofdm_mi355x
    ofdm_mi355x.load()
    return cases.Runner(ofdm_mi355x)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "despread_refusals.json")) as f:
        return json.load(f)


def test_the_fixture_is_the_table(recorded):
    assert sorted("%s/%s" % (call[5:], name) for call, of in recorded.items() for name in of) == sorted(cases.IDS)
    assert set(recorded) == set(cases.CALLS)
    flat = [r for of in recorded.values() for v in of.values() for r in (v.values() if isinstance(v, dict) else [v])]
    assert len({r[1] for r in flat}) > 200 and [0, ""] in flat
    # precedence depends on the call and on the set: the per-set combiner wants d_csi before it looks at anything else and reports
    # a missing set behind its other argument errors, the per-set stage reports it in front of them
    of = recorded["ofdm_combine_despread_alloc_frames"]
    assert of["null-d_csi-in-front-of-the-arguments-refused"] == [
        -1, "ofdm_combine_despread_alloc_frames: d_csi is required (the combiner has no meaning without it)"]
    assert of["n_seg-negative-refused"] == [-1, "ofdm_combine_despread_alloc_frames: negative count"]
    assert recorded["ofdm_combine_despread_frames"]["null-d_csi"] == [-1, "ofdm_combine_despread_frames: null d_sym or d_csi"]
    of = recorded["ofdm_dft_despread_alloc_frames"]
    assert of["n_seg-negative-refused"]["none"] == [-1, "ofdm_dft_despread_alloc_frames: no allocation set (ofdm_rx_set_allocations)"]
    assert of["n_seg-negative-refused"]["set"] == [-1, "ofdm_dft_despread_alloc_frames: negative count"]
    assert of["packed-refused"] == {"set": [-1, "ofdm_dft_despread_alloc_frames: null d_sym"],
                                    "odd": [-1, "ofdm_dft_despread_alloc_frames: packed bits need M * bits per symbol % 8 == 0"]}


@pytest.mark.parametrize("call", sorted(cases.CALLS))
def test_refusals_and_noops(runner, recorded, call):
    got = runner.run_all({call})[call]
    wrong = [(name, got[name], recorded[call][name]) for name in got if got[name] != recorded[call][name]]
    assert got and not wrong, wrong

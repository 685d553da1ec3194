"""What the codec calls of the C ABI refuse, and what they return without doing anything (-m gpu): every public call of
csrc/capi_tbcc.hip, capi_bitproc.hip, capi_turbo.hip and capi_tb.hip over the table of tests/codec_refusal_cases.py, its status and
the exact ofdm_last_error() text against tests/golden/codec_refusals.json.  The fixture is recorded from the library of the commit
in front of a change to these files (tests/golden/gen_codec_refusals.py), never from the tree under test: the order in which a call
reports its errors is behaviour.  A GPU is needed for the two handles only; no case launches a kernel."""
import json
import os

import pytest

import codec_refusal_cases as cases
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
    with open(os.path.join(GOLDEN, "codec_refusals.json")) as f:
        return json.load(f)


def test_the_fixture_is_the_table(recorded):
    assert sorted(recorded) == sorted(cases.IDS)
    assert set(call for _, call, _ in cases.CASES) == set(cases.CALLS)
    texts = {v[1] for v in recorded.values()}
    assert len(texts) > 100 and "" in texts
    # the asymmetric pair: n_seg = 2^31 without blocks is a no-op of the TBCC calls and beyond the range of the turbo calls
    assert recorded["tx_tbcc_encode_frames/asymmetric-n_seg-2^31-no-blocks"] == [0, ""]
    assert recorded["tx_turbo_encode_frames/asymmetric-n_seg-2^31-no-blocks"] == [
        -1, "ofdm_tx_turbo_encode_frames: batch beyond the kernels' index range"]


@pytest.mark.parametrize("call", sorted(cases.CALLS))
def test_refusals_and_noops(runner, recorded, call):
    wrong = []
    for cid, c, kwargs in cases.CASES:
        if c == call:
            got = runner.run(c, kwargs)
            if got != recorded[cid]:
                wrong.append((cid, got, recorded[cid]))
    assert not wrong, wrong

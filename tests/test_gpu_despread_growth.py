"""The composite calls of the four despreading families grow their workspace inside the call (-m gpu): on a handle that no
reserve call has seen, ofdm_rx_demod_frames_*despread* with 1 frame, then with 3 frames on the same handle -- the second call
grows a workspace whose pointers were valid once, so a composite that read its |H|^2 rows, tables or plan slot before its
ensure step would read freed memory here.  Both calls equal, bit for bit, the stage-by-stage path on a second handle:
demod_frames, csi_frames, then the family's stage call on the same buffers.  The smallest configuration of the families' own
test files: nfft 64, 60 data bins, QPSK, 2 branches, the set (0, 4, QPSK), (6, 6, 16-QAM)."""
import numpy as np
import pytest

from test_gpu_csi import Out, demod
from test_gpu_soft_frames import GEOM, make_frames

pytestmark = pytest.mark.gpu

N, MOD, B, SET = 64, "QPSK", 2, [(0, 4, 2), (6, 6, 4)]
WANT = ("sym", "llr", "bits", "beta", "weight")


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def frames():
    return make_frames(N, MOD, 3 * B, 8, np.random.default_rng(64))


@pytest.mark.parametrize("family", ["despread", "mrc_despread", "despread_alloc", "mrc_despread_alloc"])
def test_composite_grows_twice_and_equals_the_stage_calls(om, torch, frames, family):
    cp, Kd = GEOM[N]
    branches = B if family.startswith("mrc") else 1
    fl = frames.shape[1]
    rx, d_iq, nds = demod(om, N, MOD, frames)                # the composite's handle: no reserve call
    ref, _, _ = demod(om, N, MOD, frames)
    if family.endswith("alloc"):
        rx.set_allocations(SET)
        ref.set_allocations(SET)
    noise = dict(noise_var=[0.02, 0.03]) if branches > 1 else dict(noise_mode=om.DESPREAD_NOISE_GIVEN, noise_var=0.02)
    for nf in (1, 3):                                        # the second batch is larger: growth behind pointers that were valid
        units, room = branches * nf, branches * nf * nds * Kd

        def outs():
            o = {k: Out(torch, room * 6, torch.uint8 if k == "bits" else torch.float32) for k in WANT}
            return o, dict(d_sym_out=o["sym"].addr, d_llr=o["llr"].addr, d_bits=o["bits"].addr, bits_mode=om.BITS_UNPACKED,
                           d_beta=o["beta"].addr, d_weight=o["weight"].addr, **noise)

        (a, ka), (b, kb) = outs(), outs()
        p_eq, c_eq = Out(torch, room * 2, torch.float32), Out(torch, room * 2, torch.float32)
        assert ref.demod_frames(d_iq, units, fl, fl, p_eq.addr) == nds
        d_a = Out(torch, units * Kd, torch.float32)
        ref.csi_frames(units, d_a.addr)
        rows = (p_eq.addr, nf, nds, Kd, nds * Kd, d_a.addr, Kd, ref.csi_rho)
        if family == "despread":
            ref.dft_despread_frames(*rows, MOD, **ka)
            got = rx.demod_frames_despread(d_iq, nf, fl, fl, c_eq.addr, **kb)
        elif family == "mrc_despread":
            ref.combine_despread_frames(rows[0], B, *rows[1:], MOD, **ka)
            got = rx.demod_frames_mrc_despread(d_iq, B, nf, fl, fl, c_eq.addr, **kb)
        elif family == "despread_alloc":
            ref.dft_despread_alloc_frames(*rows, **ka)
            got = rx.demod_frames_despread_alloc(d_iq, nf, fl, fl, c_eq.addr, **kb)
        else:
            ref.combine_despread_alloc_frames(rows[0], B, *rows[1:], **ka)
            got = rx.demod_frames_mrc_despread_alloc(d_iq, B, nf, fl, fl, c_eq.addr, **kb)
        assert got == nds
        assert np.array_equal(p_eq.read().view(np.uint8), c_eq.read().view(np.uint8)), nf
        for k in WANT:
            x, y = a[k].read().view(np.uint8), b[k].read().view(np.uint8)
            assert np.array_equal(x, y), (k, nf)
        llr = a["llr"].read()
        assert np.isfinite(llr[:8]).all() and llr[:8].any(), nf  # the stage ran: the outputs are not the poison they started as

"""The symbol loop of the fused transmit kernel (`tx_modulate_kernel`; run with -m gpu).

Every other test of the kernel launches no more symbols than the chip holds workgroups (one trip per workgroup) or looks at hard
decisions only.  Here every workgroup takes at least three trips, and the output is held to two references that do not depend on
the looped launch:

  * the oracle (`orc.tx_modulate`, fp64) on sampled frames, 1e-5 norm-relative -- the tolerance of tests/test_gpu_tx_stages.py;
  * the same handle run over slices small enough for ONE trip per workgroup (what the other tests pin to the oracle), bit for
    bit over every sample: per symbol a looped trip performs the same float operations as a one-trip launch.

Sizing.  A compute unit holds at most 32 waves and a workgroup is Plan<N>::WG / 64 of them, so at most
R = n_cu * 32 / max(1, WG / 64) workgroups are resident whatever occupancy the runtime reports, and the grid is at most R.
With units >= 3 * R * SLOTS + 1 symbols the last workgroup still starts its third trip; units / SLOTS stays below n_cu * 256,
the smallest launch that could get a grid larger than the resident count.  A one-trip slice is at most n_cu * SLOTS symbols:
n_cu workgroups, never more than are resident (at least one per compute unit).

The IQ goes into a NaN-filled allocation with frames one sample further apart than they need to be: the gap sample of every
frame and the samples in front of and behind the buffer must stay NaN, and no sample of a frame may."""
from math import gcd

import numpy as np
import pytest

from conftest import relerr
from oracle import ofdm_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5
SLOTS = {64: 8, 128: 8, 256: 4, 512: 2, 1024: 1, 2048: 1, 4096: 1}          # Plan<N>::SLOTS (csrc/fft_core.hpp)
WAVES = {64: 1, 128: 1, 256: 1, 512: 1, 1024: 1, 2048: 2, 4096: 4}          # Plan<N>::WG / 64
TAIL = 2                                                                    # NaN samples kept behind the last frame


@pytest.fixture(scope="module")
def om():
    import ofdm_mi355x
    ofdm_mi355x.load()
    return ofdm_mi355x


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _min_units(N):
    """Symbols from which every workgroup of a launch takes three trips or more (module docstring)."""
    return 3 * (_n_cu() * 32 // WAVES[N]) * SLOTS[N] + 1


def _grid(wgs, resident, slots, SD):
    """csrc/tx_grid.hpp: tx_modulate_grid below the large-launch regime, restated (used to pick frames to sample only)."""
    g = min(wgs, resident)
    if g < wgs and slots == 1:
        while g > 1 and gcd(g, SD) != 1:
            g -= 1
    return g


def _first_difference(a, b, lead, stride, L):
    import torch
    idx = int(torch.nonzero((a != b).any(dim=1))[0]) - lead
    f, s = divmod(idx, stride)
    return "first difference at frame %d, symbol %d, sample %d: looped %r, one trip %r" % (
        f, s // L, s % L, a[idx + lead].view(torch.float32).tolist(), b[idx + lead].view(torch.float32).tolist())


def _check_loop(om, N, cp, Kd, pattern, mod, n_sym, n_frames, packed=False, odd_bits=False, lead=2, seed=1):
    """Looped launch of n_frames x n_sym symbols against one-trip launches (bit for bit, all samples) and the oracle (sampled).
    `lead` samples of NaN lie in front of the output (1: the output starts 8 bytes into a 16-byte line), `odd_bits` puts the bit
    stream at an odd address.  Returns the tensors the caller may look at further."""
    import torch
    S, D = pattern
    SD, L, slots, n_cu = S + D, N + cp, SLOTS[N], _n_cu()
    units = n_frames * n_sym
    wgs = -(-units // slots)
    assert units >= _min_units(N) and wgs < n_cu * 256                      # three trips or more, resident-sized grid
    bps = orc.BITS_PER_SYMBOL[mod]
    Ks = N - 2
    tx = om.TxEngine(N, cp, Ks, Kd, pattern, mod)
    nb = tx.bits_per_frame(n_sym)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(seed)
    if packed:
        assert nb % 8 == 0
        nbytes, mode = nb // 8, om.BITS_PACKED
        raw = torch.zeros(n_frames * nbytes + 16, dtype=torch.uint8, device=dev)
        raw[int(odd_bits):int(odd_bits) + n_frames * nbytes] = torch.randint(0, 256, (n_frames * nbytes,), dtype=torch.uint8, device=dev, generator=gen)
    else:
        nbytes, mode = nb, om.BITS_UNPACKED
        raw = torch.zeros(n_frames * nbytes + 16, dtype=torch.uint8, device=dev)
        raw[int(odd_bits):int(odd_bits) + n_frames * nbytes] = torch.randint(0, 2, (n_frames * nbytes,), dtype=torch.uint8, device=dev, generator=gen)
    p_bits = raw.data_ptr() + int(odd_bits)
    assert (p_bits & 3) == (1 if odd_bits else 0)
    fl = n_sym * L
    stride = fl + 1
    total = lead + n_frames * stride + TAIL
    looped = torch.full((total, 2), float("nan"), dtype=torch.float32, device=dev)
    single = torch.full((total, 2), float("nan"), dtype=torch.float32, device=dev)
    assert (looped.data_ptr() & 15) == 0 and (single.data_ptr() & 15) == 0
    torch.cuda.synchronize()

    tx.modulate_frames(p_bits, n_frames, n_sym, looped.data_ptr() + lead * 8, frame_stride=stride, bits_mode=mode)

    # one trip per workgroup: at most n_cu workgroups a launch
    cap = n_cu * slots
    p_single = single.data_ptr() + lead * 8
    if n_sym <= cap:                                                        # whole frames
        per = cap // n_sym
        for f0 in range(0, n_frames, per):
            nf = min(per, n_frames - f0)
            assert -(-nf * n_sym // slots) <= n_cu
            tx.modulate_frames(p_bits + f0 * nbytes, nf, n_sym, p_single + f0 * stride * 8, frame_stride=stride, bits_mode=mode)
    else:                                                                   # whole patterns of a long frame: a pattern starts
        assert not packed and cap >= SD                                     # like a frame does, with its first sync symbol
        chunk = cap // SD * SD
        for f in range(n_frames):
            for s0 in range(0, n_sym, chunk):
                ns = min(chunk, n_sym - s0)
                tx.modulate_frames(p_bits + f * nbytes + s0 // SD * D * Kd * bps, 1, ns, p_single + (f * stride + s0 * L) * 8,
                                   frame_stride=ns * L, bits_mode=mode)
    torch.cuda.synchronize()

    a, b = looped.view(torch.int32), single.view(torch.int32)
    if not torch.equal(a, b):
        pytest.fail(_first_difference(a, b, lead, stride, L))
    # nothing outside the frames, everything inside them
    frames = looped[lead:lead + n_frames * stride].view(n_frames, stride, 2)
    assert bool(torch.isnan(looped[:lead]).all()) and bool(torch.isnan(looped[lead + n_frames * stride:]).all())
    assert bool(torch.isnan(frames[:, fl]).all())
    assert not bool(torch.isnan(frames[:, :fl]).any())
    # every sync symbol is the handle's, exactly
    sym = frames[:, :fl].unflatten(1, (n_sym, L))                           # [frame][symbol][sample][re, im], a view
    sync = torch.from_numpy(tx.sync_symbol().view(np.float32).reshape(S, L, 2)).to(dev)
    for r in range(S):
        assert bool((sym[:, r::SD] == sync[r]).all()), "sync symbol %d" % r

    # the oracle on sampled pieces (frame, first symbol, symbols): whole frames, or pairs of patterns of a long frame
    rng = np.random.default_rng(seed)
    piece = n_sym if n_sym <= cap else 2 * SD
    def at(unit):
        f, s = divmod(min(unit, units - 1), n_sym)
        return (f, 0) if piece == n_sym else (f, s // SD * SD)
    picks = {at(0), at(units - 1)}
    picks |= {at(_grid(wgs, n_cu * k, slots, SD) * slots) for k in range(1, 32 // WAVES[N] + 1)}       # unit g, any occupancy
    picks |= {at(int(u)) for u in rng.integers(0, units, 12)}
    worst = 0.0
    for f, s0 in sorted(picks):
        ns = min(piece, n_sym - s0)
        b0 = s0 // SD * D * Kd * bps
        nbp = tx.data_symbols(ns) * Kd * bps
        if packed:
            fb = np.unpackbits(raw[int(odd_bits) + f * nbytes:int(odd_bits) + (f + 1) * nbytes].cpu().numpy())
        else:
            fb = raw[int(odd_bits) + f * nbytes + b0:int(odd_bits) + f * nbytes + b0 + nbp].cpu().numpy()
        ref = orc.tx_modulate(fb, N, cp, Ks, Kd, ns, synch_dat=pattern, modulation=mod)
        got = frames[f, s0 * L:(s0 + ns) * L].cpu().numpy().view(np.complex64).ravel()
        e = relerr(got, ref)
        worst = max(worst, e)
        assert e < TOL, "frame %d, symbols %d..%d: %.3g" % (f, s0, s0 + ns, e)
    print("N %d %s: %d symbols, %d pieces against the oracle, worst %.3g" % (N, mod, units, len(picks), worst))
    return tx, sym


def _frames_for(N, n_sym, uneven=False):
    """Fewest frames of n_sym symbols that reach _min_units(N); `uneven`: a symbol count that is no multiple of SLOTS."""
    n = -(-_min_units(N) // n_sym)
    while uneven and (n * n_sym) % SLOTS[N] == 0:
        n += 1
    return n


@pytest.mark.parametrize("N,cp,Kd,mod,packed", [(1024, 72, 600, "QPSK", False), (2048, 144, 1200, "16QAM", True),
                                                (4096, 288, 2400, "64QAM", True)])
def test_many_short_frames_one_symbol_per_workgroup(om, N, cp, Kd, mod, packed):
    """Frames of 9 symbols of a [1, 3] pattern (the frame ends inside a pattern, and the stride is no multiple of 9 in general:
    the symbol index wraps into the next frame); 4-byte-aligned two-bit fetch, packed 16-QAM, packed 64-QAM (the instantiation
    compiled for three waves per SIMD)."""
    _check_loop(om, N, cp, Kd, (1, 3), mod, 9, _frames_for(N, 9), packed=packed, seed=N)


def test_two_long_frames_stride_shorter_than_a_frame(om):
    """Two frames longer than the grid: the frame index only ever advances by the wrap.  [2, 3] pattern, 4-byte-aligned
    six-bit fetch; the frame ends after the two sync and two data symbols of a last, partial pattern."""
    N = 1024
    n_sym = -(-_min_units(N) // 2)
    while n_sym % 5 != 4:
        n_sym += 1
    tx, _ = _check_loop(om, N, 72, 600, (2, 3), "64QAM", n_sym, 2, seed=7)
    assert tx.bits_per_frame(n_sym) % 4 == 0
    assert n_sym > _n_cu() * 32                                             # stride <= resident workgroups < n_sym


def test_bit_by_bit_fetch_and_misaligned_output_in_the_loop(om):
    """Unpacked 16-QAM at an odd address (read bit by bit) and the output 8 bytes into a 16-byte line (with the odd frame stride
    every second frame starts aligned, the others take the 8-byte stores)."""
    _check_loop(om, 2048, 144, 1200, (1, 3), "16QAM", 9, _frames_for(2048, 9), odd_bits=True, lead=1, seed=11)


@pytest.mark.parametrize("N,cp,Kd,mod,packed", [(64, 15, 60, "BPSK", True), (256, 18, 180, "16QAM", False)])
def test_several_symbols_per_workgroup(om, N, cp, Kd, mod, packed):
    """Below 1024-pt a workgroup holds SLOTS symbols side by side and transforms its sync symbols itself.  The symbol count is
    no multiple of SLOTS: the last workgroup's last trip has idle slots.  64-pt: packed BPSK (bit-by-bit fetch of a packed
    stream) and an odd cp (scalar stores); 256-pt: unpacked 16-QAM."""
    n_frames = _frames_for(N, 10, uneven=True)
    assert (n_frames * 10) % SLOTS[N] != 0
    _check_loop(om, N, cp, Kd, (2, 3), mod, 10, n_frames, packed=packed, seed=N)


def test_pattern_length_sharing_a_factor_with_the_resident_count(om):
    """[1, 1]: with an even grid half of the workgroups would meet sync symbols only; whatever grid the launcher picks, every
    data symbol has to be produced and every sync symbol has to be the handle's (checked for every frame in _check_loop)."""
    _, sym = _check_loop(om, 1024, 72, 600, (1, 1), "QPSK", 8, _frames_for(1024, 8), seed=13)
    assert sym.shape[1] == 8

"""tests/mrc_despread_alloc_ref.py -- the contract "receive diversity for multi-user allocations of DFT-spread OFDM" restated --
pinned without a GPU: one allocation over the whole row is mrc_despread_ref on the row; every user gets the gain, the weight and
the unbiased symbols of its own columns; a user's outputs do not depend on the other users, their channels or the gaps; a branch
erased in one user's columns is an erasure for that user alone; beta and weight are laid out per row.  Last, the link case of
mrc_despread_alloc_cases.py on the oracle's receiver."""
import math

import numpy as np

import dft_alloc_ref
import dft_spread_ref
import mrc_despread_alloc_ref as aref
import mrc_despread_ref as ref
from oracle import ofdm_oracle as orc

NAME = {2: "QPSK", 4: "16QAM", 6: "64QAM"}
RHO = np.float32(0.03)


def make(rng, B, n_seg, rows, row_len, allocs, gain=None, sig=0.02):
    """-> z [B][n_seg][rows][row_len] complex64, a [B][n_seg][row_len] float32, sigma2 [B][n_seg], x the sent rows per allocation
    [u][n_seg][rows][M_u]: every allocation a user of its own through B channels and one-tap MMSE equalisers; gaps hold noise"""
    z = (rng.standard_normal((B, n_seg, rows, row_len)) + 1j * rng.standard_normal((B, n_seg, rows, row_len))).astype(np.complex64)
    a = rng.uniform(0.1, 1.0, (B, n_seg, row_len)).astype(np.float32)
    s2 = np.full((B, n_seg), sig)
    sent = []
    for u, (start, M, bps) in enumerate(allocs):
        xs = np.zeros((n_seg, rows, M), complex)
        for s in range(n_seg):
            xs[s] = orc.map_bits(rng.integers(0, 2, rows * M * bps), NAME[bps]).reshape(rows, M)
            X = dft_spread_ref.spread(xs[s])
            for b in range(B):
                av = rng.uniform(0.5, 2.0, M) * (1.0 if gain is None else gain[u])
                w = (rng.standard_normal((rows, M)) + 1j * rng.standard_normal((rows, M))) * math.sqrt(s2[b, s] / 2)
                z[b, s, :, start:start + M] = (av / (av + RHO)) * (X + w / np.sqrt(av))
                a[b, s, start:start + M] = av
        sent.append(xs)
    return z, a, s2, sent


def same(p, q):
    return np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8))


def test_one_allocation_over_the_whole_row_is_the_single_size_stage():
    rng = np.random.default_rng(1)
    B, n_seg, rows, M = 3, 2, 4, 60
    allocs = [(0, M, 4)]
    z, a, s2, _ = make(rng, B, n_seg, rows, M, allocs)
    got = aref.combine_despread_alloc(z, a, allocs, RHO, s2)
    for s in range(n_seg):
        seg = ref.combine_despread_segment(z[:, s], a[:, s], RHO, s2[:, s])
        n = rows * M
        assert same(got["comb"][s * n:(s + 1) * n], seg["comb"].ravel())
        assert same(got["sym"][s * n:(s + 1) * n], seg["sym"].ravel())
        assert same(got["beta"][s * rows:(s + 1) * rows], seg["beta32"]) and same(got["weight"][s * rows:(s + 1) * rows], seg["weight32"])
        l, b = ref.segment_llr(seg, 4)
        assert same(got["llr"][s * n * 4:(s + 1) * n * 4], l) and same(got["bits"][s * n * 4:(s + 1) * n * 4], b)


def test_every_user_gets_the_weights_and_unbiased_symbols_of_its_own_columns():
    rng = np.random.default_rng(2)
    B, n_seg, rows, row_len = 2, 1, 40, 64
    allocs = [(2, 24, 2), (30, 30, 2)]                       # gaps at both ends and inside
    z, a, s2, sent = make(rng, B, n_seg, rows, row_len, allocs, gain=(1.0, 0.01), sig=0.02)
    got = aref.combine_despread_alloc(z, a, allocs, RHO, s2)
    at, total = aref.row_layout(len(allocs), n_seg, rows)
    assert got["beta"].size == total
    beta = [got["beta"][at(u, 0, 0):at(u, 0, 0) + rows] for u in range(2)]
    weight = [got["weight"][at(u, 0, 0):at(u, 0, 0) + rows] for u in range(2)]
    assert (beta[0] > 0.95).all() and (beta[1] < 0.8).all() and (beta[1] > 0).all()       # the weak user's own, smaller gain
    assert weight[0].min() > 10 * weight[1].max()
    so = aref.layout(allocs, n_seg, rows)[0]
    for u, (start, M, _) in enumerate(allocs):
        sym = got["sym"][so[u]:so[u] + rows * M].reshape(rows, M)
        x = sent[u][0]
        bias = np.vdot(x, sym).real / np.vdot(x, x).real                                  # unbiased: the projection on x is 1
        # the projection of rows*M unit-power symbols with error variance 1/weight has the standard deviation
        # 1/sqrt(2 rows M weight); the bound is four of them
        assert abs(bias - 1) < 4.0 / math.sqrt(2 * rows * M * np.mean(weight[u])), (u, bias)
        err = np.mean(np.abs(sym - x) ** 2)                                               # the weight is 1 / the error variance
        assert 0.7 < err * np.mean(weight[u]) < 1.4, (u, err, np.mean(weight[u]))
        # the same numbers as the single-size restatement on the gathered columns
        seg = ref.combine_despread_segment(z[:, 0, :, start:start + M], a[:, 0, start:start + M], RHO, s2[:, 0])
        assert same(seg["beta32"], beta[u]) and same(seg["weight32"], weight[u]) and same(seg["sym"], sym)


def test_a_user_does_not_depend_on_the_other_users_or_the_gaps():
    rng = np.random.default_rng(3)
    B, n_seg, rows, row_len = 3, 2, 3, 81
    allocs = [(1, 25, 4), (27, 1, 2), (31, 45, 6)]
    z, a, s2, _ = make(rng, B, n_seg, rows, row_len, allocs)
    base = aref.combine_despread_alloc(z, a, allocs, RHO, s2)
    so, lo, _, _ = aref.layout(allocs, n_seg, rows)
    at, _ = aref.row_layout(len(allocs), n_seg, rows)

    def block(res, u):
        _, M, bps = allocs[u]
        n = n_seg * rows * M
        return [res["sym"][so[u]:so[u] + n], res["comb"][so[u]:so[u] + n], res["llr"][lo[u]:lo[u] + n * bps],
                res["bits"][lo[u]:lo[u] + n * bps], res["beta"][at(u, 0, 0):at(u + 1, 0, 0)], res["weight"][at(u, 0, 0):at(u + 1, 0, 0)]]

    covered = np.zeros(row_len, bool)
    for start, M, _ in allocs:
        covered[start:start + M] = True
    z2, a2 = z.copy(), a.copy()
    z2[..., ~covered] = complex(np.nan, np.nan)              # the gaps are never read for data
    a2[..., ~covered] = np.nan
    res = aref.combine_despread_alloc(z2, a2, allocs, RHO, s2)
    assert all(same(p, q) for u in range(3) for p, q in zip(block(res, u), block(base, u)))
    for v, (start, M, _) in enumerate(allocs):
        for what in ("data", "channel"):
            z3, a3 = z.copy(), a.copy()
            if what == "data":
                z3[..., start:start + M] *= np.complex64(0.5 + 0.25j)
            else:
                a3[..., start:start + M] *= np.float32(0.7)
            res = aref.combine_despread_alloc(z3, a3, allocs, RHO, s2)
            for u in range(3):
                keeps = all(same(p, q) for p, q in zip(block(res, u), block(base, u)))
                assert keeps == (u != v), (u, v, what)
    # the list in another order: the same blocks, permuted
    perm = allocs[1:] + allocs[:1]
    res = aref.combine_despread_alloc(z, a, perm, RHO, s2)
    so2 = aref.layout(perm, n_seg, rows)[0]
    for k, (start, M, _) in enumerate(perm):
        u = allocs.index(perm[k])
        n = n_seg * rows * M
        assert same(res["sym"][so2[k]:so2[k] + n], base["sym"][so[u]:so[u] + n])
        assert same(res["beta"][at(k, 0, 0):at(k + 1, 0, 0)], base["beta"][at(u, 0, 0):at(u + 1, 0, 0)])


def test_a_branch_erased_in_one_users_columns_is_an_erasure_for_that_user_alone():
    rng = np.random.default_rng(4)
    B, n_seg, rows, row_len = 2, 1, 3, 60
    allocs = [(0, 36, 4), (36, 24, 4)]
    z, a, s2, _ = make(rng, B, n_seg, rows, row_len, allocs)
    base = aref.combine_despread_alloc(z, a, allocs, RHO, s2)
    a2 = a.copy()
    a2[1, 0, 36:60] = 0                                      # branch 1 has no usable entry in user 1's columns
    got = aref.combine_despread_alloc(z, a2, allocs, RHO, s2)
    assert not got["segs"][1][0]["took"][1].any() and got["segs"][1][0]["took"][0].all()
    assert got["segs"][0][0]["took"].all()
    one = ref.combine_despread_segment(z[:1, 0, :, 36:60], a[:1, 0, 36:60], RHO, s2[:1, 0])   # user 1: branch 0 alone
    assert same(got["segs"][1][0]["sym"], one["sym"]) and same(got["segs"][1][0]["beta32"], one["beta32"])
    assert (got["segs"][1][0]["beta32"] < base["segs"][1][0]["beta32"]).all()
    assert same(got["segs"][0][0]["sym"], base["segs"][0][0]["sym"]) and same(got["segs"][0][0]["weight32"], base["segs"][0][0]["weight32"])
    a2[0, 0, 36:60] = np.nan                                 # every branch: user 1's rows are erasures, user 0 carries on
    z2 = z.copy()
    z2[:, 0, 1, 0:36] = 0                                    # and row 1 of user 0 has nothing in any branch
    got = aref.combine_despread_alloc(z2, a2, allocs, RHO, s2)
    at, _ = aref.row_layout(2, n_seg, rows)
    assert not got["beta"][at(1, 0, 0):].any() and not got["weight"][at(1, 0, 0):].any()
    assert not got["sym"][rows * 36:].any() and not got["llr"][rows * 36 * 4:].any()
    assert got["segs"][1][0]["erased"].all()
    b0 = got["beta"][:rows]
    assert b0[0] > 0 and b0[2] > 0 and b0[1] == 0 and list(got["segs"][0][0]["erased"]) == [False, True, False]
    assert np.isfinite(got["sym"]).all() and np.isfinite(got["llr"]).all()


def test_layout_of_beta_and_weight():
    at, total = aref.row_layout(3, 4, 5)
    assert total == 60 and at(0, 0, 0) == 0 and at(0, 0, 4) == 4 and at(0, 1, 0) == 5 and at(1, 0, 0) == 20 and at(2, 3, 4) == 59
    seen = sorted(at(u, s, r) for u in range(3) for s in range(4) for r in range(5))
    assert seen == list(range(60))
    rng = np.random.default_rng(5)
    allocs = [(0, 12, 2), (12, 24, 4)]
    z, a, s2, _ = make(rng, 2, 2, 3, 36, allocs)
    got = aref.combine_despread_alloc(z, a, allocs, RHO, s2)
    at, _ = aref.row_layout(2, 2, 3)
    for u in range(2):
        for s in range(2):
            for r in range(3):
                assert got["beta"][at(u, s, r)] == got["segs"][u][s]["beta32"][r]
                assert got["weight"][at(u, s, r)] == got["segs"][u][s]["weight32"][r]
    so, lo, bo, tot = aref.layout(allocs, 2, 3)
    assert so == [0, 72] and lo == [0, 144] and tot[:2] == (216, 720) and got["sym"].size == 216 and got["llr"].size == 720


# ------------------------------------------------------------------------------------------ the link case, on the reference alone
def received_frames(noise_var):
    """the case's frames through the allocation precoder and the oracle's receiver branch by branch -> (z [B][frames][9][60]
    complex64 equalised rows, a [B][frames][60] float32 channel powers, info bits)"""
    import channel_ref
    import csi_ref
    import mrc_despread_alloc_cases as ac
    import turbo_ref
    info = ac.info_bits()
    coded = turbo_ref.encode_segments(info, ac.F1, ac.F2, ac.SEG_BITS)
    rows = [r for r in range(ac.N_SYM) if r % 4 != 3]
    bins = orc.bins_p(ac.KD, ac.N)
    tx = []
    for f in range(ac.N_FRAMES):
        spread = dft_alloc_ref.spread_alloc(orc.map_bits(coded[f], ac.MOD).reshape(ac.N_DSYM, ac.KD), ac.ALLOCS)
        tx.append(orc.tx_modulate(None, ac.N, ac.CP, ac.KS, ac.KD, ac.N_SYM, modulation=ac.MOD, data_symbols=spread))
    z = np.zeros((ac.N_BRANCH, ac.N_FRAMES, ac.N_DSYM, ac.KD), np.complex64)
    a = np.zeros((ac.N_BRANCH, ac.N_FRAMES, ac.KD), np.float32)
    for b in range(ac.N_BRANCH):
        noise = channel_ref.noise(ac.SEED_NOISE + b, ac.N_FRAMES, ac.FRAME_LEN, noise_var)
        for f in range(ac.N_FRAMES):
            y = np.convolve(tx[f], ac.TAPS[b])[:ac.FRAME_LEN - ac.LEAD]
            x = np.zeros(ac.FRAME_LEN, complex)
            x[ac.LEAD:ac.LEAD + len(y)] = y
            x += noise[f]
            o = orc.RxOracle(ac.N_SYM, ac.N, ac.CP, ac.KS, [1, 3], ac.KD, ac.SNR_ARG, ac.GATE, force_fp64=True)
            o.work(x.astype(np.complex64), np.zeros(ac.FRAME_LEN, np.complex64))
            z[b, f] = o.est_data_freq[rows]
            a[b, f] = csi_ref.csi_row(o.est_chan_freq_P[0].astype(np.complex64), bins)
    return z, a, info


def link_result(noise_var):
    """-> blocks lost of 64 at this noise level: {"combined", "branch 0 alone", "branch 1 alone"}.  The combined stage and the
    single-branch allocation stage (dft_alloc_ref, noise given) both take noise_var as the variance of every branch; the LLRs of
    both are put back into row order before the decoder."""
    import mrc_despread_alloc_cases as ac
    import turbo_ref
    rho = np.float32(1.0 / 10.0 ** (ac.SNR_ARG / 20.0))
    z, a, info = received_frames(noise_var)
    B, n = ac.N_BRANCH, ac.N_FRAMES
    got = aref.combine_despread_alloc(z, a, ac.ALLOCS, rho, np.full((B, n), noise_var))
    assert all(seg["usable"].all() for per in got["segs"] for seg in per)
    llr = {"combined": ac.rows_from_blocks(got["llr"])}
    for b in range(B):
        blocks = [[] for _ in ac.ALLOCS]
        for f in range(n):
            for u, (sym, wt, _) in enumerate(dft_alloc_ref.despread_alloc_segment(z[b, f], a[b, f], ac.ALLOCS, rho, noise_var)):
                assert wt["usable"]
                blocks[u].append(dft_spread_ref.outputs_from(sym.astype(np.complex64), wt["weight32"], ac.MOD)[0])
        llr["branch %d alone" % b] = ac.rows_from_blocks(np.concatenate([np.concatenate(v) for v in blocks]))
    lost = {}
    for k, v in llr.items():
        bits, _ = turbo_ref.decode_segments(v, 1, ac.K, ac.F1, ac.F2, ac.N_ITER)
        lost[k] = int((bits != info).any(axis=(1, 2)).sum())
    return lost


def test_rows_from_blocks_puts_the_llrs_back_into_row_order():
    import mrc_despread_alloc_cases as ac
    n, rows = 2, 3
    rowwise = np.arange(n * rows * ac.KD * 4, dtype=np.float32).reshape(n, rows, ac.KD, 4)
    blocks = np.concatenate([rowwise[:, :, s:s + M, :].ravel() for s, M, _ in ac.ALLOCS])
    assert np.array_equal(ac.rows_from_blocks(blocks, n, rows), rowwise.reshape(n, -1))


def test_link_case_on_the_reference():
    import mrc_despread_alloc_cases as ac
    assert dft_alloc_ref.check_set(ac.ALLOCS, ac.KD) is None and sum(a[1] for a in ac.ALLOCS) == ac.KD
    res = {name: link_result(nv) for name, nv in (("level", ac.NOISE_VAR), ("1 dB up", ac.NOISE_VAR_1DB))}
    print("blocks lost of %d: %r" % (ac.N_FRAMES, res))
    assert res["level"]["combined"] == 0 and res["1 dB up"]["combined"] == 0
    assert res["level"]["branch 0 alone"] >= ac.MIN_LOST_ALONE and res["level"]["branch 1 alone"] >= ac.MIN_LOST_ALONE
    assert res["level"] == ac.LOST_AT_LEVEL

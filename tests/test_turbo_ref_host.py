"""tests/turbo_ref.py, the yardstick of the turbo kernels, pinned without a GPU and by means that do not share its code: the
encoder against polynomial arithmetic over GF(2), the interleaver against its definition, the SISO against a dense (max, +) matrix
evaluation in float64, the decoder against the transmitted bits, and the operating point of the GPU test's inputs."""
import numpy as np
import pytest

import turbo_cases as tc
import turbo_ref as tr

FB = np.array([1, 0, 1, 1])                                  # 1 + D^2 + D^3, lowest power first
FF = np.array([1, 1, 0, 1])                                  # 1 + D + D^3


def polymul2(a, b):
    return np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64)) % 2


# ------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("K", (40, 64, 120, 512))
def test_parity_times_feedback_equals_input_times_feedforward_and_the_registers_end_in_zero(K):
    rng = np.random.default_rng(K)
    c = rng.integers(0, 2, (5, K)).astype(np.uint8)
    f1, f2 = tc.QPP[K]
    e = tr.encode(c, f1, f2)
    pi = tr.qpp(K, f1, f2)
    for enc, src in ((0, c), (1, c[:, pi])):
        z, tail, end = tr.rsc(src)
        assert not end.any()
        assert np.array_equal(z, e[:, 1 + enc:3 * K:3]) and np.array_equal(tail, e[:, 3 * K + 6 * enc:3 * K + 6 * enc + 6])
        for n in range(5):
            u = np.concatenate([src[n], tail[n, 0::2]])      # information bits, then the three transmitted x
            zz = np.concatenate([z[n], tail[n, 1::2]])
            assert np.array_equal(polymul2(zz, FB), polymul2(u, FF))
    assert np.array_equal(e[:, 0:3 * K:3], c)


def test_stream_layout_of_the_tail():
    """TS 36.212 5.1.3.2.2: d0, d1, d2 at k = K .. K+3 hold x_K z_K x_{K+1} | z_{K+1} x_{K+2} z_{K+2} | the same primed"""
    K = 40
    c = np.random.default_rng(3).integers(0, 2, (4, K)).astype(np.uint8)
    f1, f2 = tc.QPP[K]
    e = tr.encode(c, f1, f2).reshape(4, K + 4, 3)
    _, t1, _ = tr.rsc(c)
    _, t2, _ = tr.rsc(c[:, tr.qpp(K, f1, f2)])
    x, z, xp, zp = t1[:, 0::2], t1[:, 1::2], t2[:, 0::2], t2[:, 1::2]
    d0, d1, d2 = e[:, K:, 0], e[:, K:, 1], e[:, K:, 2]
    assert np.array_equal(d0, np.stack([x[:, 0], z[:, 1], xp[:, 0], zp[:, 1]], 1))
    assert np.array_equal(d1, np.stack([z[:, 0], x[:, 2], zp[:, 0], xp[:, 2]], 1))
    assert np.array_equal(d2, np.stack([x[:, 1], z[:, 2], xp[:, 1], zp[:, 2]], 1))


def test_encoder_is_linear_and_its_impulse_response_is_the_series_of_the_transfer_function():
    K = 64
    f1, f2 = tc.QPP[K]
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 2, (2, 6, K)).astype(np.uint8)
    assert np.array_equal(tr.encode(a ^ b, f1, f2), tr.encode(a, f1, f2) ^ tr.encode(b, f1, f2))
    series = np.zeros(K, np.int64)                           # FF / FB by long division
    rem = np.zeros(K + 4, np.int64)
    rem[:4] = FF
    for k in range(K):
        series[k] = rem[k]
        if rem[k]:
            rem[k:k + 4] ^= FB
    assert np.array_equal(series[3:17], np.tile(series[3:10], 2))         # period 7 behind the transient
    for pos in (0, 1, 9, K - 1):
        c = np.zeros((1, K), np.uint8)
        c[0, pos] = 1
        z, _, _ = tr.rsc(c)
        assert np.array_equal(z[0, pos:], series[:K - pos]) and not z[0, :pos].any()


# ------------------------------------------------------------------------------------------ interleaver
def test_qpp_triples():
    for K, (f1, f2) in tc.QPP.items():
        assert tr.qpp_check(K, f1, f2), (K, f1, f2)
    assert tr.qpp_check(*tc.IDENTITY) and np.array_equal(tr.qpp(*tc.IDENTITY), np.arange(40))
    for bad in ((40, 2, 10), (40, 0, 0), (64, 2, 0), (48, 7, 8), (44, 3, 10), (32, 3, 8), (6152, 3, 10), (40, 40, 0), (40, 3, 40),
                (40, -1, 0)):
        assert not tr.qpp_check(*bad), bad
    for K in (72, 520):
        assert tc.QPP[K][1] == 0 and np.gcd(tc.QPP[K][0], K) == 1


@pytest.mark.parametrize("K", sorted(tc.QPP))
def test_incremental_qpp_equals_the_formula(K):
    """pi(i+1) = pi(i) + g(i), g(i+1) = g(i) + 2 f2 (mod K), and the stride-8 form the decoder's tile load uses"""
    f1, f2 = tc.QPP[K]
    pi = tr.qpp(K, f1, f2)
    p, g = 0, (f1 + f2) % K
    for i in range(K):
        assert p == pi[i]
        p, g = (p + g) % K, (g + 2 * f2) % K
    for i0 in (0, 3, 7):
        p, g = int(pi[i0]), (8 * f1 + 64 * f2 + 16 * f2 * i0) % K
        for i in range(i0, K, 8):
            assert p == pi[i]
            p, g = (p + g) % K, (g + 128 * f2) % K


# ------------------------------------------------------------------------------------------ SISO against a dense evaluation
NEG = -np.inf


def dense_siso(ls, la, lp, t):
    """One block in float64, no normalisation: every step is an 8 x 8 (max, +) matrix T_k[s][s'] = gamma_k of the branch s -> s'
    (-inf where there is none); alpha_k = alpha_0 T_0 .. T_{k-1}, beta_k = T_k .. T_{K-1} beta_K, and M_u is the best whole path
    through a branch of input u at step k."""
    K = len(ls)
    x = ls.astype(np.float64) + la.astype(np.float64)
    lp = lp.astype(np.float64)
    t = t.astype(np.float64)
    sig = (1.0, -1.0)

    def branch(s, u):
        r1, r2, r3 = s >> 2, (s >> 1) & 1, s & 1
        a = u ^ r2 ^ r3
        return 4 * a + (s >> 1), a ^ r1 ^ r3

    def mat(k, only_u=None):
        T = np.full((8, 8), NEG)
        for s in range(8):
            for u in (0, 1):
                if only_u is None or u == only_u:
                    nxt, z = branch(s, u)
                    T[s, nxt] = sig[u] * x[k] + sig[z] * lp[k]
        return T

    def vec_mat(v, T):
        return np.max(v[:, None] + T, axis=0)

    def mat_vec(T, v):
        return np.max(T + v[None, :], axis=1)

    beta_K = np.zeros(8)
    for s in range(8):
        cur = s
        for j in range(3):
            r1, r2, r3 = cur >> 2, (cur >> 1) & 1, cur & 1
            beta_K[s] += sig[r2 ^ r3] * t[2 * j] + sig[r1 ^ r3] * t[2 * j + 1]
            cur >>= 1
    alpha = [np.array([0.0] + [NEG] * 7)]
    for k in range(K):
        alpha.append(vec_mat(alpha[-1], mat(k)))
    beta = [None] * K + [beta_K]
    for k in range(K - 1, -1, -1):
        beta[k] = mat_vec(mat(k), beta[k + 1])
    post = np.empty(K)
    for k in range(K):
        M = [np.max(alpha[k] + mat_vec(mat(k, u), beta[k + 1])) for u in (0, 1)]
        post[k] = 0.5 * (M[0] - M[1])
    return post, 0.75 * (post - x)


def dense_decode(l, K, f1, f2, n_iter):
    pi = tr.qpp(K, f1, f2)
    l = l.astype(np.float64)
    ls, lp1, lp2 = l[0:3 * K:3], l[1:3 * K:3], l[2:3 * K:3]
    la1 = np.zeros(K)
    for _ in range(n_iter):
        _, e1 = dense_siso(ls, la1, lp1, l[3 * K:3 * K + 6])
        post2, e2 = dense_siso(ls[pi], e1[pi], lp2, l[3 * K + 6:])
        la1 = np.empty(K)
        la1[pi] = e2
    out = np.empty(K)
    out[pi] = post2
    return out


@pytest.mark.parametrize("K,lo,hi", ((40, -1, 2), (40, -3, 4), (56, -2, 3)))
def test_siso_equals_the_dense_evaluation_on_small_integers(K, lo, hi):
    """On small-integer LLRs every float32 operation of the contract is exact (0.5 and 0.75 add at most three fractional bits
    per half-iteration), so the normalised float32 recursion must equal the unnormalised float64 one exactly."""
    f1, f2 = tc.QPP[K]
    llr = np.random.default_rng(K + hi).integers(lo, hi, (3, 3 * K + 12)).astype(np.float32)
    for n_iter in (1, 2):
        bits, out = tr.decode(llr, f1, f2, n_iter)
        for n in range(3):
            want = dense_decode(llr[n], K, f1, f2, n_iter)
            assert np.array_equal(out[n].astype(np.float64), want), (n_iter, n)
            assert np.array_equal(bits[n], want < 0)
    l = llr[:1]
    post, ext = tr.siso(l[:, 0:3 * K:3], np.zeros((1, K), np.float32), l[:, 1:3 * K:3], l[:, 3 * K:3 * K + 6])
    dp, de = dense_siso(l[0, 0:3 * K:3], np.zeros(K), l[0, 1:3 * K:3], l[0, 3 * K:3 * K + 6])
    assert np.array_equal(post[0], dp) and np.array_equal(ext[0], de)


# ------------------------------------------------------------------------------------------ decoding
@pytest.mark.parametrize("K", tc.ENC_KS)
def test_noiseless_decoding_returns_the_payload(K):
    f1, f2 = tc.QPP[K]
    c = np.random.default_rng(K).integers(0, 2, (2, K)).astype(np.uint8)
    bits, out = tr.decode((1.0 - 2.0 * tr.encode(c, f1, f2)).astype(np.float32), f1, f2, 1)
    assert np.array_equal(bits, c) and np.all(np.isfinite(out)) and out.dtype == np.float32


def test_non_finite_inputs_count_as_zero_and_all_zero_decides_zero():
    K = 40
    llr, _ = tc.noisy_blocks(K, 4)
    dirty = llr.copy()
    idx = np.random.default_rng(1).integers(0, 3 * K + 12, 30)
    dirty[:, idx[:10]], dirty[:, idx[10:20]], dirty[:, idx[20:]] = np.nan, np.inf, -np.inf
    clean = dirty.copy()
    clean[:, idx] = 0
    for a, b in zip(tr.decode(dirty, *tc.QPP[K], 2), tr.decode(clean, *tc.QPP[K], 2)):
        assert np.array_equal(a, b)
    bits, out = tr.decode(np.zeros((1, 3 * K + 12), np.float32), *tc.QPP[K], 3)
    assert not bits.any() and not out.any()


@pytest.mark.parametrize("K", tc.DEC_KS)
def test_operating_point_of_the_gpu_inputs(K):
    """The very blocks tests/test_gpu_turbo.py decodes: 10 % .. 60 % of them wrong at n_iter = 1, strictly fewer at n_iter = 6,
    so that the comparison on the GPU covers wrong decisions as well as clean ones."""
    wrong = {}
    for n_iter in tc.DEC_ITERS:
        _, c, bits, out = tc.decoded(K, n_iter)
        wrong[n_iter] = int(np.any(bits != c, axis=1).sum())
        assert np.all(np.isfinite(out))
    print("K=%d Es/N0=%.1f dB: wrong blocks of %d at n_iter 1/2/6: %s" % (K, tc.ESN0_DB[K], tc.DEC_BLOCKS, wrong))
    assert 0.10 * tc.DEC_BLOCKS <= wrong[1] <= 0.60 * tc.DEC_BLOCKS
    assert wrong[6] < wrong[1]


def test_edge_blocks_reach_ties_and_zero_signs():
    K = 40
    llr = tc.edge_blocks(K)
    bits, out = tr.decode(llr, *tc.QPP[K], 2)
    assert not bits[2].any() and not bits[6].any() and not out[2].any()
    assert np.all(np.isfinite(out))
    # integer LLRs keep every metric on a coarse dyadic grid (exact arithmetic), which is what makes the candidates of a max tie
    assert np.array_equal(out[3] * 4096, np.round(out[3] * 4096)) and len(np.unique(out[3])) < K
    assert np.signbit(llr[5]).any() and (llr[5] == 0).any() and (np.abs(llr[5]) < 1.2e-38).any()

"""Pins tests/turbo_es_ref.py (the incremental reference with freeze masks) by the definition in include/ofdm_mi355x.h, which
shares no control flow with it: turbo_ref.decode at every n_iter, and the first n in min_iter .. max_iter whose bits pass
lte_bits_ref.crc_check.  Then asserts, on the reference alone, the operating points tests/test_gpu_turbo_es.py relies on.
No GPU."""
import numpy as np
import pytest

import lte_bits_ref as lb
import turbo_cases as tc
import turbo_es_cases as ec
import turbo_es_ref as er
import turbo_ref as tr


def by_definition(llr, f1, f2, kind, min_iter, max_iter):
    n = llr.shape[0]
    per_n = {it: tr.decode(llr, f1, f2, it) for it in range(min_iter, max_iter + 1)}
    bits = np.zeros((n, (llr.shape[1] - 12) // 3), np.uint8)
    out = np.zeros(bits.shape, np.float32)
    iters, ok = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for b in range(n):
        stop = max_iter
        for it in range(min_iter, max_iter + 1):
            passed, _, _ = lb.crc_check(per_n[it][0][b:b + 1], kind, 0)
            if passed[0]:
                stop, ok[b] = it, 1
                break
        bits[b], out[b], iters[b] = per_n[stop][0][b], per_n[stop][1][b], stop
    return bits, out, iters, ok


def same(got, want):
    for g, w, name in zip(got, want, ("bits", "llr", "iters", "crc_ok")):
        if name == "llr":
            g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("K", ec.SPREAD_KS)
def test_incremental_reference_equals_the_definition_on_the_spread_cases(K):
    llr, _ = ec.spread(K)
    for lo, hi in ec.ITER_PAIRS:
        same(ec.spread_ref(K, lo, hi), by_definition(llr, *tc.QPP[K], lb.CRC24B, lo, hi))


@pytest.mark.parametrize("kind", (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8))
def test_incremental_reference_equals_the_definition_for_every_kind(kind):
    K, llr, _, ref = ec.kind_case(kind)
    same(ref, by_definition(llr, *tc.QPP[K], kind, 1, ec.MAX_ITER))


def test_incremental_reference_equals_the_definition_on_edge_values_and_false_passes():
    K = 56
    llr = tc.edge_blocks(K)
    for lo, hi in ((1, 3), (2, 3)):
        ref = er.decode_es(llr, *tc.QPP[K], lb.CRC24B, lo, hi)
        same(ref, by_definition(llr, *tc.QPP[K], lb.CRC24B, lo, hi))
        # all-zero and all-NaN LLRs decide all zeros, whose remainder is zero: a false pass at min_iter
        assert ref[2][2] == lo and ref[2][6] == lo and ref[3][2] == 1 and ref[3][6] == 1 and not ref[0][2].any() and not ref[0][6].any()
    llr, _, ref = ec.false_pass()
    same(ref, by_definition(llr, *tc.QPP[ec.FALSE_PASS_K], lb.CRC8, 1, ec.MAX_ITER))


@pytest.mark.parametrize("K", ec.SPREAD_KS)
def test_spread_cases_hold_every_stopping_behaviour_in_one_group(K):
    """within one 8-block group: a block that stops at 1, one that stops strictly between 1 and 6, one that never passes"""
    _, _, iters, ok = ec.spread_ref(K, 1, ec.MAX_ITER)
    print("K=%d iters %s crc_ok %s" % (K, iters.tolist(), ok.tolist()))
    assert any(np.any((iters[g] == 1) & (ok[g] == 1)) and np.any((iters[g] > 1) & (iters[g] < ec.MAX_ITER) & (ok[g] == 1)) and
               np.any(ok[g] == 0) for g in (slice(0, 8), slice(8, 16)))
    assert np.all(iters[ok == 0] == ec.MAX_ITER)


def test_crc8_false_pass_case_has_a_wrong_block_that_passes():
    llr, sent, (bits, _, iters, ok) = ec.false_pass()
    hit = (ok == 1) & np.any(bits != sent, axis=1)
    print("CRC8 on noise-only LLRs, seed %d: blocks %s pass wrongly at iterations %s" % (ec.FALSE_PASS_SEED, np.flatnonzero(hit).tolist(),
                                                                                        iters[hit].tolist()))
    assert hit.any()


def test_kind_cases_stop_early_and_the_wrong_kind_never_passes():
    for kind in (lb.CRC24A, lb.CRC24B, lb.CRC16, lb.CRC8):
        K, llr, info, (bits, _, iters, ok) = ec.kind_case(kind)
        assert np.any(iters[ok == 1] < ec.MAX_ITER) and np.any(iters > 1)
    K, llr, _, _ = ec.kind_case(lb.CRC24B)
    _, _, iters, ok = er.decode_es(llr, *tc.QPP[K], lb.CRC24A, 1, ec.MAX_ITER)
    assert not ok.any() and np.all(iters == ec.MAX_ITER)


@pytest.mark.parametrize("K", (40, 72))
def test_neighbour_wave_and_flipped_bits(K):
    for pos in (0, 5):
        _, _, iters, ok = er.decode_es(ec.neighbour_wave(K, pos), *tc.QPP[K], lb.CRC24B, 1, ec.MAX_ITER)
        want = np.ones(8, np.uint8)
        want[pos] = ec.MAX_ITER
        assert np.array_equal(iters, want) and ok[pos] == 0 and ok.sum() == 7
    for at in (0, K - 25, K - 24, K - 1):
        llr = ec.flipped_bit(K, at)
        bits, _, iters, ok = er.decode_es(llr, *tc.QPP[K], lb.CRC24B, 1, 1)
        assert ok[0] == 0 and iters[0] == 1
        clean = llr.copy()
        clean[0, 3 * at] = -np.sign(clean[0, 3 * at])
        assert er.decode_es(clean, *tc.QPP[K], lb.CRC24B, 1, 1)[3][0] == 1

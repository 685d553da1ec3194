// dft_rows_launch.hpp -- what the despreading row kernels of DFT-spread OFDM share on the host: the step from a call's run-time
// (size class, llr or bits wanted, modulation) to the <MOD, MORE, CAP> instance of a kernel, and the classes of an allocation set
// with the lookup a workgroup makes in one (alloc_of, the one __device__ function here: it reads the class that make_class builds).
// dft_spread.hip and mrc_despread.hip use the instance dispatch alone, dft_alloc.hip and mrc_despread_alloc.hip all of it.
#pragma once
#include "ofdm_launch.hpp"

namespace ofdm {

namespace {

// An instance of a row kernel: MORE: llr and / or bits are wanted, at MOD bits per symbol (sym alone: MOD = 2); CAP >= M, the
// occupancy classes of dft_mixed.hpp.
template <int MOD, bool MORE, int CAP>
struct RowInst {
    static constexpr int mod = MOD, cap = CAP;
    static constexpr bool more = MORE;
};

// fn(RowInst<...>{}) for the instance that serves (small: M <= DFT_SMALL_M, more, mod); fn launches and returns the error
template <int CAP, class Fn>
hipError_t with_row_instance_cap(bool more, int mod, Fn fn) {
    if (!more) return fn(RowInst<2, false, CAP>{});
    switch (mod) {
        case 2: return fn(RowInst<2, true, CAP>{});
        case 4: return fn(RowInst<4, true, CAP>{});
        case 6: return fn(RowInst<6, true, CAP>{});
    }
    return hipErrorInvalidValue;
}
template <class Fn>
hipError_t with_row_instance(bool small, bool more, int mod, Fn fn) {
    return small ? with_row_instance_cap<DFT_SMALL_M>(more, mod, fn) : with_row_instance_cap<DFT_MAX_M>(more, mod, fn);
}
// fn for each of the eight instances (the *_prepare() calls); the first error
template <class Fn>
hipError_t each_row_instance(Fn fn) {
    hipError_t e = hipSuccess;
    for (int small = 1; small >= 0; --small)
        for (int mod = 0; mod <= 6 && e == hipSuccess; mod += 2) e = with_row_instance(small, mod != 0, mod, fn);
    return e;
}

// the class's allocation of workgroup b: k with end[k-1] <= b < end[k]; uniform over the workgroup
__device__ __forceinline__ int alloc_of(const DftAllocClass& c, unsigned b, unsigned& first) {
    int k = 0;
    first = 0;
    while (k < c.n - 1 && b >= c.end[k]) first = c.end[k++];
    return k;
}

// the allocations of h_set[0 .. n) of one size class and (mod != 0) one modulation, with their workgroups: units (segments, or 1)
// times the groups of `rows`
inline DftAllocClass make_class(const DftAllocDesc* h_set, int n, int64_t units, int64_t rows, bool small, int mod) {
    DftAllocClass c{};
    uint64_t end = 0;
    for (int u = 0; u < n; ++u) {
        if ((h_set[u].pl.M <= DFT_SMALL_M) != small || (mod != 0 && h_set[u].mod != mod)) continue;
        const int rpg = h_set[u].pl.rows_per_group;
        end += uint64_t(units) * uint64_t((rows + rpg - 1) / rpg);
        c.idx[c.n] = uint8_t(u);
        c.end[c.n++] = unsigned(end);
    }
    return c;
}

// fn(class, small, mod) for every class present in the set, the small sizes first: the size class and, where `more`, the
// modulation (mod = 2 otherwise).  Stops at the first error.
template <class Fn>
hipError_t for_each_alloc_class(const DftAllocDesc* h_set, int n, int64_t units, int64_t rows, bool more, Fn fn) {
    for (int small = 1; small >= 0; --small) {
        for (int mod = 2; mod <= (more ? 6 : 2); mod += 2) {
            const DftAllocClass c = make_class(h_set, n, units, rows, bool(small), more ? mod : 0);
            if (c.n == 0) continue;
            const hipError_t e = fn(c, bool(small), mod);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace

}  // namespace ofdm

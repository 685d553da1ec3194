// demap_rules.hip -- the fused de-mapper's hard-decision functions (csrc/demap_hard.hpp) run on the device, one output per variant.
//
//   demap_rules MOD in.bin outdir
//     in.bin   complex64[n], n % 4 == 0 (symbols, in the order the groups of pack4 / pairs of pack2 take them)
//     writes   outdir/<variant>.bin, uint8[n * MOD]: every variant's bits unpacked to one bit per byte, MSB first per symbol
//     prints   the variant names, one per line
//
// Variants (MOD in {1, 2, 4, 6}):
//   hard         hard_bits<MOD>, one symbol per lane (the rule every other variant must reproduce)
//   pack4_asm    pack4<MOD, true>   / pack4_c   pack4<MOD, false>   groups of 4 (fused packed bits, N <= 512)
//   pack2_asm    pack2<MOD, true>   / pack2_c   pack2<MOD, false>   pairs (fused packed bits, dense mapping, N >= 1024)
//   store_p_asm  store_bits<MOD, 1, true> / store_p_c  store_bits<MOD, 1, false>   packed bytes (MOD even only)
//   store_u      store_bits<MOD, 2>                                 one bit per byte, groups of 4
//   store_pair_u store_bits_pair_unpacked<MOD>                      one bit per byte, pairs
// Built with the library's own flags (csrc/Makefile) so the inline assembly runs as it does in the product.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "demap_hard.hpp"

using ofdm::cf;

#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));             \
            std::exit(2);                                                            \
        }                                                                            \
    } while (0)

template <int MOD>
__global__ void k_hard(const cf* z, int64_t n, uint8_t* out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned hb = ofdm::hard_bits<MOD>(z[i]);
    for (int b = 0; b < MOD; ++b) out[i * MOD + b] = uint8_t((hb >> (MOD - 1 - b)) & 1u);
}

// `w` holds G*MOD bits, MSB first
template <int MOD, int G>
__device__ void unpack_word(uint8_t* out, unsigned w) {
    for (int k = 0; k < G * MOD; ++k) out[k] = uint8_t((w >> (G * MOD - 1 - k)) & 1u);
}

template <int MOD, bool ASMB>
__global__ void k_pack4(const cf* z, int64_t n, uint8_t* out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= n / 4) return;
    const cf zz[4] = {z[4 * g], z[4 * g + 1], z[4 * g + 2], z[4 * g + 3]};
    unpack_word<MOD, 4>(out + g * 4 * MOD, ofdm::pack4<MOD, ASMB>(zz));
}

template <int MOD, bool ASMB>
__global__ void k_pack2(const cf* z, int64_t n, uint8_t* out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= n / 2) return;
    const cf zz[2] = {z[2 * g], z[2 * g + 1]};
    unpack_word<MOD, 2>(out + g * 2 * MOD, ofdm::pack2<MOD, ASMB>(zz));
}

// packed output: n * MOD / 8 bytes
template <int MOD, bool ASMB>
__global__ void k_store_packed(const cf* z, int64_t n, uint8_t* out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= n / 4) return;
    const cf zz[4] = {z[4 * g], z[4 * g + 1], z[4 * g + 2], z[4 * g + 3]};
    ofdm::store_bits<MOD, 1, ASMB>(out, 4 * g, zz, 4);
}

template <int MOD>
__global__ void k_store_unpacked(const cf* z, int64_t n, uint8_t* out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= n / 4) return;
    const cf zz[4] = {z[4 * g], z[4 * g + 1], z[4 * g + 2], z[4 * g + 3]};
    ofdm::store_bits<MOD, 2>(out, 4 * g, zz, 4);
}

template <int MOD>
__global__ void k_store_pair(const cf* z, int64_t n, uint8_t* out) {
    const int64_t g = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (g >= n / 2) return;
    const cf zz[2] = {z[2 * g], z[2 * g + 1]};
    ofdm::store_bits_pair_unpacked<MOD>(out, unsigned(2 * g), zz);
}

struct Run {
    const cf* d_z;
    int64_t n;
    uint8_t* d_out;
    std::string dir;

    // launches `k` over `items` lanes into a zeroed buffer of `out_bytes`, writes the bits (unpacked if `packed`) to dir/name.bin
    template <typename K>
    void variant(const char* name, K k, int64_t items, int64_t out_bytes, bool packed) {
        CHECK(hipMemset(d_out, 0xAB, size_t(out_bytes)));
        const unsigned grid = unsigned((items + 255) / 256);
        hipLaunchKernelGGL(k, dim3(grid), dim3(256), 0, 0, d_z, n, d_out);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        std::vector<uint8_t> h(static_cast<size_t>(out_bytes));
        CHECK(hipMemcpy(h.data(), d_out, size_t(out_bytes), hipMemcpyDeviceToHost));
        std::vector<uint8_t> bits;
        if (packed) {
            bits.resize(size_t(out_bytes) * 8);
            for (size_t i = 0; i < bits.size(); ++i) bits[i] = uint8_t((h[i >> 3] >> (7 - (i & 7))) & 1u);
        } else {
            bits = h;
        }
        const std::string path = dir + "/" + name + ".bin";
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f || std::fwrite(bits.data(), 1, bits.size(), f) != bits.size()) {
            std::fprintf(stderr, "cannot write %s\n", path.c_str());
            std::exit(2);
        }
        std::fclose(f);
        std::printf("%s\n", name);
    }
};

template <int MOD>
void run_all(Run& r) {
    const int64_t n = r.n, nb = n * MOD;
    r.variant("hard", k_hard<MOD>, n, nb, false);
    r.variant("pack4_asm", k_pack4<MOD, true>, n / 4, nb, false);
    r.variant("pack4_c", k_pack4<MOD, false>, n / 4, nb, false);
    r.variant("pack2_asm", k_pack2<MOD, true>, n / 2, nb, false);
    r.variant("pack2_c", k_pack2<MOD, false>, n / 2, nb, false);
    if constexpr (MOD % 2 == 0) {                      // packed bytes: MOD even only (capi_internal.hpp: demod_bad_args refuses BPSK packed)
        r.variant("store_p_asm", k_store_packed<MOD, true>, n / 4, nb / 8, true);
        r.variant("store_p_c", k_store_packed<MOD, false>, n / 4, nb / 8, true);
    }
    r.variant("store_u", k_store_unpacked<MOD>, n / 4, nb, false);
    r.variant("store_pair_u", k_store_pair<MOD>, n / 2, nb, false);
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s MOD in.bin outdir\n", argv[0]);
        return 1;
    }
    const int mod = std::atoi(argv[1]);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 1;
    }
    std::vector<cf> z;
    float xy[2];
    while (std::fread(xy, sizeof(float), 2, f) == 2) z.push_back(cf{xy[0], xy[1]});
    std::fclose(f);
    const int64_t n = int64_t(z.size());
    if (n == 0 || n % 4 != 0 || (mod != 1 && mod != 2 && mod != 4 && mod != 6)) {
        std::fprintf(stderr, "need MOD in {1,2,4,6} and a non-empty symbol count divisible by 4 (got MOD=%d, n=%lld)\n", mod,
                     (long long)n);
        return 1;
    }
    Run r{nullptr, n, nullptr, argv[3]};
    cf* d_z = nullptr;
    CHECK(hipMalloc(&d_z, size_t(n) * sizeof(cf)));
    CHECK(hipMemcpy(d_z, z.data(), size_t(n) * sizeof(cf), hipMemcpyHostToDevice));
    CHECK(hipMalloc(&r.d_out, size_t(n) * 6));
    r.d_z = d_z;
    switch (mod) {
        case 1: run_all<1>(r); break;
        case 2: run_all<2>(r); break;
        case 4: run_all<4>(r); break;
        default: run_all<6>(r); break;
    }
    CHECK(hipFree(d_z));
    CHECK(hipFree(r.d_out));
    return 0;
}

// capi_common.hip -- what belongs to no handle: the error text, the host-built tables (twiddles, Zadoff-Chu, scan kernel),
// the derived receiver constants, and the handle-free calls (device memory, sharding, probe, bit-error count).
#include "capi_internal.hpp"

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

std::vector<cf> make_twiddles(int n) {
    std::vector<cf> t(n);
    for (int j = 0; j < n; ++j) {
        const double a = -2.0 * M_PI * double(j) / double(n);
        t[j] = cf{float(std::cos(a)), float(std::sin(a))};
    }
    return t;
}

// SynchAndChanEst.py:52-59 / SynchSignal.py:23-30 (root 23) ; synch_and_chan_est.py:54-64 (root 37)
std::vector<cf> make_zc(int mm, int root, int parity_of) {
    std::vector<cf> z(mm);
    for (int n = 0; n < mm; ++n) {
        const double x0 = double(n), x1 = double(n + 1);
        const double q = (parity_of % 2 == 0) ? (x0 * x0 / 2.0) : (x0 * x1 / 2.0);
        const double a = -(2.0 * M_PI / double(mm)) * double(root) * q;
        z[n] = cf{float(std::cos(a)), float(std::sin(a))};
    }
    return z;
}

// G[m] = sum_i e^{+j 2pi m k_i / N} conj(zc_i), m = 0..N (G[N] = G[0]): the kernel of the screened sync search's recurrence
// (rx_sync_scan_kernel).  Unnormalised inverse DFT of the sync symbol's conjugated grid row, iterative radix-2 in double.
std::vector<cf> make_scan_table(int N, int Ks, const std::vector<cf>& zc) {
    std::vector<std::complex<double>> g(size_t(N), {0.0, 0.0});
    const int h = Ks / 2;
    for (int i = 0; i < Ks; ++i) {
        const int k = i < h ? N - h + i : i - h + 1;                    // binsP(Ks) (SynchAndChanEst.py:38-41)
        g[size_t(k)] = std::conj(std::complex<double>(zc[size_t(i)].x, zc[size_t(i)].y));
    }
    for (int i = 1, j = 0; i < N; ++i) {                                // bit reversal
        int bit = N >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(g[size_t(i)], g[size_t(j)]);
    }
    for (int len = 2; len <= N; len <<= 1) {
        const double ang = 2.0 * M_PI / double(len);                    // e^{+j..}: inverse transform
        for (int i = 0; i < N; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const std::complex<double> w(std::cos(ang * k), std::sin(ang * k));
                const auto x = g[size_t(i + k)], y = g[size_t(i + k + len / 2)] * w;
                g[size_t(i + k)] = x + y;
                g[size_t(i + k + len / 2)] = x - y;
            }
    }
    std::vector<cf> out(size_t(N) + 2);
    double gmax = 0.0;
    for (int m = 0; m <= N; ++m) {
        out[size_t(m)] = cf{float(g[size_t(m % N)].real()), float(g[size_t(m % N)].imag())};
        gmax = std::max(gmax, std::abs(g[size_t(m % N)]));
    }
    out[size_t(N) + 1] = cf{float(gmax * (1.0 + 1e-6)), 0.f};          // max |G[m]|: the checkpoint bound of the screened search
    return out;
}

// Derived constants of a receiver configuration; returns the Zadoff-Chu root.
int fill_rxdev(const ofdm_rx_cfg& cfg, RxDev& d) {
    const ofdm_rx_cfg* c = &cfg;
    const int N = c->nfft, Ks = c->num_synch_bins, Kd = c->num_data_bins, S = c->synch_S;
    const int MM = S * Ks;
    d.nfft = N;
    d.cp = c->cp_len;
    d.L = N + c->cp_len;
    d.Ks = Ks;
    d.Kd = Kd;
    d.S = S;
    d.D = c->synch_D;
    d.MM = MM;
    d.bps = c->modulation;
    double snr_ls, snr_eq, snr_data, gate;
    int root;
    if (c->compat == OFDM_COMPAT_UTSA) {
        const double snr_lin = std::pow(10.0, c->snr / 20.0);     // SynchAndChanEst.py:99 (sic: /20)
        snr_ls = snr_lin;                                          // :180
        snr_eq = c->snr;                                           // :214 uses the raw argument
        snr_data = snr_lin;                                        // :245
        gate = c->scale_factor_gate;                               // :166
        d.stride = 1;                                              // :77
        root = 23;                                                 // :52
    } else {
        snr_ls = snr_eq = snr_data = c->snr;                       // synch_and_chan_est.py:184,217,247
        gate = 0.4;                                                // :170
        d.stride = c->cp_len - 1;                                  // :81
        root = 37;                                                 // :54
    }
    d.gate_mm = float(gate * double(MM));
    d.inv_ls = float(1.0 / (double(S) * (1.0 + 1.0 / snr_ls)));
    d.inv_snr_data = float(1.0 / snr_data);
    d.inv_snr_eqsync = float(1.0 / snr_eq);
    return root;
}

// The tables every receiver handle owns: twiddles, and the ZC sequence with its lane-order copy stored behind it; `d` (nfft, Ks,
// S, MM already filled) gets the pointers to them.
int upload_rx_tables(RxDev& d, cf** d_tw, cf** d_zc, const std::vector<cf>& zc) {
    std::vector<cf> both = zc;
    const auto zcp = rx_zc_lane_table(d.nfft, d.Ks, d.S, zc.data());
    both.insert(both.end(), zcp.begin(), zcp.end());
    int rc = upload(d_tw, make_twiddles(d.nfft));
    if (rc == OFDM_OK) rc = upload(d_zc, both);
    if (rc != OFDM_OK) return rc;
    d.tw = *d_tw;
    d.zc = *d_zc;
    d.zcp = *d_zc + d.MM;
    return rc;
}

extern "C" {

int ofdm_abi_version(void) { return OFDM_ABI_VERSION; }

int ofdm_shard_frames(int64_t n_frames_total, int32_t world, int32_t rank, int64_t* first, int64_t* count) {
    if (!first || !count || world < 1 || rank < 0 || rank >= world || n_frames_total < 0)
        return fail(OFDM_ERR_INVALID, "ofdm_shard_frames: bad argument");
    if (n_frames_total % world)
        return fail(OFDM_ERR_INVALID, "n_frames_total=%lld is not a multiple of world=%d", (long long)n_frames_total, int(world));
    *count = n_frames_total / world;
    *first = int64_t(rank) * *count;
    return OFDM_OK;
}
const char* ofdm_last_error(void) { return g_last_error.c_str(); }

int ofdm_device_malloc(int32_t device, void** d_ptr, int64_t bytes) {
    if (!d_ptr || bytes < 0) return fail(OFDM_ERR_INVALID, "ofdm_device_malloc: bad argument");
    HIP_TRY(hipSetDevice(device));
    hipError_t e = hipMalloc(d_ptr, size_t(bytes));
    if (e != hipSuccess) return fail(OFDM_ERR_NOMEM, "hipMalloc(%lld): %s", (long long)bytes, hipGetErrorString(e));
    return OFDM_OK;
}
int ofdm_device_free(int32_t device, void* d_ptr) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(d_ptr));
    return OFDM_OK;
}
int ofdm_memcpy_h2d(int32_t device, void* d_dst, const void* h_src, int64_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(d_dst, h_src, size_t(bytes), hipMemcpyHostToDevice));
    return OFDM_OK;
}
int ofdm_memcpy_d2h(int32_t device, void* h_dst, const void* d_src, int64_t bytes) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(h_dst, d_src, size_t(bytes), hipMemcpyDeviceToHost));
    return OFDM_OK;
}
int ofdm_device_synchronize(int32_t device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    return OFDM_OK;
}

int ofdm_bandwidth_probe(int32_t device, const void* d_in, void* d_out, int64_t bytes, int32_t mode, int32_t sym_in_bytes,
                         int32_t gap_bytes, int32_t sym_out_bytes, int64_t n_sym, void* stream) {
    if (!d_in || !d_out || bytes < 0 || (bytes & 15) || (sym_in_bytes & 15) || (gap_bytes & 15) || (sym_out_bytes & 15))
        return fail(OFDM_ERR_INVALID, "ofdm_bandwidth_probe: sizes must be multiples of 16 bytes");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_probe(d_in, d_out, bytes / 16, mode, sym_in_bytes / 16, gap_bytes / 16, sym_out_bytes / 16, n_sym,
                         static_cast<hipStream_t>(stream)));
    return OFDM_OK;
}

int ofdm_count_bit_errors(int32_t device, const uint8_t* d_a, const uint8_t* d_b, int64_t n_bytes, uint64_t* d_count, void* stream) {
    if (!d_count || n_bytes < 0 || (n_bytes > 0 && (!d_a || !d_b))) return fail(OFDM_ERR_INVALID, "ofdm_count_bit_errors: bad argument");
    if (n_bytes > (int64_t(1) << 40)) return fail(OFDM_ERR_INVALID, "ofdm_count_bit_errors: more than 2^40 bytes per call");
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_bit_errors(d_a, d_b, n_bytes, reinterpret_cast<unsigned long long*>(d_count), static_cast<hipStream_t>(stream)));
    return OFDM_OK;
}

}  // extern "C"

// tdec_crc_api.hip -- the host code of the frame check (include/crc.h): the
// table cache and the launches of k_crc (tdec_crc.hip), and the generator call that takes the
// caller's info bits (k_workload_faded<TxArgs>, tdec_workload.hip).  Included at the end of
// tdec_api.hip: it needs the handle's internals and the generators' argument helpers.
#include <map>
#include <tuple>

#include "crc.h"

namespace {

struct CrcKind {
    int r;
    uint32_t poly, init;
};

bool crc_kind(int kind, CrcKind &k) {
    if (kind == CRC_KIND16) k = {16, 0x1021u, 0xFFFFu};
    else if (kind == CRC_KIND32) k = {32, 0x04C11DB7u, 0xFFFFFFFFu};
    else return false;
    return true;
}

// v x mod g (v: r bits)
uint32_t crc_times_x(uint32_t v, const CrcKind &k) {
    const uint32_t top = (v >> (k.r - 1)) & 1u, mask = k.r == 32 ? 0xFFFFFFFFu : (1u << k.r) - 1u;
    return ((v << 1) & mask) ^ (top ? k.poly : 0u);
}

// The device table of a (device, kind, L) and the two constants that go with it.  Entries
// live until the process ends: a few KB each, one per row length in use.
struct CrcTable {
    uint32_t *d = nullptr;
    uint32_t c_verify = 0, c_attach = 0;   // init x^L, init x^(L-r) mod g
};
std::mutex g_crc_mu;
std::map<std::tuple<int, int, int>, CrcTable> g_crc_tables;

// The cached table, built and uploaded on the first call (the one call that allocates and
// synchronises; refused under stream capture).
int crc_table(int device, int kind, const CrcKind &k, int L, hipStream_t st, CrcTable &out) {
    std::lock_guard<std::mutex> lock(g_crc_mu);
    const auto key = std::make_tuple(device, kind, L);
    const auto it = g_crc_tables.find(key);
    if (it != g_crc_tables.end()) {
        out = it->second;
        return 0;
    }
    if (capturing(st))
        return fail(TDEC_EUNSUPPORTED, "the first CRC call for a (device, kind, row_bits) uploads its table: make it "
                                       "outside stream capture");
    std::vector<uint32_t> t(L);
    uint32_t v = k.poly;                   // x^r mod g
    for (int j = L - 1; j >= 0; --j) {
        t[j] = v;                          // x^(L-1-j) x^r mod g
        v = crc_times_x(v, k);
    }
    CrcTable e;
    e.c_verify = e.c_attach = k.init;
    for (int i = 0; i < L; ++i) {
        e.c_verify = crc_times_x(e.c_verify, k);
        if (i < L - k.r) e.c_attach = crc_times_x(e.c_attach, k);
    }
    HIPCHK(hipMalloc(&e.d, sizeof(uint32_t) * L));
    if (hipMemcpy(e.d, t.data(), sizeof(uint32_t) * L, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(e.d);
        return fail(TDEC_EHIP, "hipMemcpy failed (CRC table)");
    }
    g_crc_tables[key] = e;
    out = e;
    return 0;
}

// attach (d_ok null) or verify over B rows of E
template <typename E>
int crc_launch(int device, int kind, long B, int L, const E *d_in, E *d_out, int32_t *d_ok, uint32_t *d_rem,
               void *stream) {
    const bool attach = d_out != nullptr;
    CrcKind k;
    if (!crc_kind(kind, k)) return fail(TDEC_EINVAL, "unknown CRC kind (CRC_KIND16 or CRC_KIND32)");
    if (L % 8 != 0 || L <= k.r || L > CRC_MAX_ROW_BITS || B < 0)
        return fail(TDEC_EINVAL, "bad CRC arguments (row_bits a multiple of 8, r < row_bits <= 2048; B >= 0)");
    if (B == 0) return 0;
    if (!d_in || (!attach && !d_ok)) return fail(TDEC_EINVAL, "bad CRC arguments (null pointer)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(TDEC_EHIP, "no such HIP device");
    Guard g(device);
    CrcTable t;
    if (int rc = crc_table(device, kind, k, L, (hipStream_t)stream, t)) return rc;
    CrcArgs a{};
    a.in = d_in, a.out = d_out, a.B = B, a.L = L, a.r = k.r;
    a.c0 = attach ? t.c_attach : t.c_verify;
    a.table = t.d, a.ok = d_ok, a.rem = d_rem;
    a.vec = (uintptr_t)d_in % (sizeof(E) == 4 ? 16 : 8) == 0;
    const long blocks = std::min<long>((B + CRC_ROWS_PER_BLOCK - 1) / CRC_ROWS_PER_BLOCK, CRC_MAX_BLOCKS);
    const dim3 grid((unsigned)blocks), block(CRC_WAVES * 64);
    if constexpr (sizeof(E) == 4) hipLaunchKernelGGL((k_crc<int32_t, false>), grid, block, 0, (hipStream_t)stream, a);
    else if (attach) hipLaunchKernelGGL((k_crc<uint8_t, true>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((k_crc<uint8_t, false>), grid, block, 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return 0;
}

static_assert(CRC_WAVES == CRC_ROWS_PER_BLOCK && CRC_MAX_L == CRC_MAX_ROW_BITS, "crc.h states the kernel's launch");

}  // namespace

extern "C" {

int crc_attach_dev(int device, int kind, long B, int row_bits, uint8_t *d_rows_u8, void *stream) {
    return crc_launch<uint8_t>(device, kind, B, row_bits, d_rows_u8, d_rows_u8, nullptr, nullptr, stream);
}

int crc_check_dev(int device, int kind, long B, int row_bits, const int32_t *d_bits_i32, int32_t *d_ok,
                  uint32_t *d_rem, void *stream) {
    return crc_launch<int32_t>(device, kind, B, row_bits, d_bits_i32, nullptr, d_ok, d_rem, stream);
}

int crc_check_u8_dev(int device, int kind, long B, int row_bits, const uint8_t *d_bits_u8, int32_t *d_ok,
                     uint32_t *d_rem, void *stream) {
    return crc_launch<uint8_t>(device, kind, B, row_bits, d_bits_u8, nullptr, d_ok, d_rem, stream);
}

int crc_workload_tx_dev(tdec_t *h, int B, int tx, int64_t cw0, uint64_t seed, const float *cons_iq, int M, int bps,
                        double sigma, int fading, double rician_k, int coh, const uint8_t *d_bits_in, float *d_syms,
                        float *d_h, void *stream) {
    if (!h || B < 0 || cw0 < 0 || tx < 0 || tx > 65535)
        return fail(TDEC_EINVAL, "bad workload arguments (0 <= tx <= 65535)");
    if (B == 0) return 0;
    if (!d_bits_in || (uintptr_t)d_bits_in % 8 != 0)
        return fail(TDEC_EINVAL, "bad workload arguments (info bits: a non-null, 8-byte aligned pointer)");
    WorkloadArgs a;
    TxArgs f{};
    if (!symbol_args(a, h, B, cw0, seed, cons_iq, M, bps, sigma, d_syms, nullptr) ||
        (fading && !fade_args(f, rician_k, coh, a.S, d_h)))
        return fail(TDEC_EINVAL, BAD_FADING);
    a.bits_in = d_bits_in;
    f.tx = tx;
    f.fade = fading != 0;
    return workload_launch(h, B, k_workload_faded<TxArgs>, stream, a, f);
}

}  // extern "C"

// Kernel-level entry points of include/t3_engine.h (t3k_*): host buffers in, host buffers out.
// They run exactly the kernels the engine runs, so the parity tests can check each kernel against the
// oracle's function of the same name through the C ABI.
#include <cstring>
#include <string>
#include <vector>

#include "t3_kernels.h"

using namespace t3;

namespace {
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes, bool zero = false) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess && zero) e = hipMemset(p, 0, bytes ? bytes : 16);
        return e;
    }
    hipError_t from(const void* h, size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(p, h, bytes, hipMemcpyHostToDevice);
        return e;
    }
    template <typename T> T* as() { return reinterpret_cast<T*>(p); }
};
bool have_device() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess && n > 0; }
// the launchers and the pool bytes per block of a storage format (T3EngineConfig.kv_cache_dtype: 0 bf16, 1 FP8 E4M3, 4 MXFP4)
size_t kv_block_bytes(int fmt) { return fmt == 4 ? (size_t)KV4_BLOCK_BYTES : (size_t)KV_BLOCK_ELEMS * (fmt == 1 ? 1 : 2); }
hipError_t rope_kv_of(int fmt, const RopeArgs& a) { return fmt == 4 ? launch_rope_kv_fp4(a, nullptr) : fmt == 1 ? launch_rope_kv_fp8(a, nullptr) : launch_rope_kv(a, nullptr); }
hipError_t attention_of(int fmt, const AttnArgs& a) { return fmt == 4 ? launch_attention_fp4(a, nullptr) : fmt == 1 ? launch_attention_fp8(a, nullptr) : launch_attention(a, nullptr); }
hipError_t kv_gather_of(int fmt, const uint16_t* kv, const int* rec, int stride, int rows, uint16_t* out) {
    return fmt == 4 ? launch_kv_gather_fp4(kv, rec, stride, rows, out, nullptr) : fmt == 1 ? launch_kv_gather_fp8(kv, rec, stride, rows, out, nullptr) : launch_kv_gather(kv, rec, stride, rows, out, nullptr);
}
}  // namespace

#define K_TRY(expr) do { if ((expr) != hipSuccess) return T3_E_DEVICE; } while (0)

extern "C" int t3k_set_prefill_rows(int32_t rows) { set_pgemm_min_rows(rows); return T3_OK; }
extern "C" int t3k_set_prefill_wide_rows(int32_t rows) { set_pgemm_wide_rows(rows); return T3_OK; }

extern "C" int t3k_gemm(const void* x, const void* w, int32_t M, int32_t K, int32_t N, float* out, int32_t mt, int32_t nw) {
    if (!x || !w || !out || M <= 0 || N <= 0 || (nw != 4 && nw != 16) || !(nw == 4 ? K == D : ((K == D || K == F) && N % 16 == 0))) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    const int Npad = (N + 15) / 16 * 16;
    std::vector<uint16_t> packed((size_t)Npad * K);
    pack_weight((const uint16_t*)w, N, K, Npad, packed.data());
    DevBuf dx, dw, dout;
    K_TRY(dx.from(x, (size_t)M * K * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2)); K_TRY(dout.alloc((size_t)M * N * 4, true));
    GemmArgs a{dx.as<uint16_t>(), dw.as<uint4>(), M, K, N, dout.p, N, nw, 0, nullptr};
    K_TRY(launch_gemm(a, EPI_F32, mt > 0 ? mt : choose_mt(M, Npad / 16, nw, false), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* RMSNorm folded into the GEMM: out[r][n] = rstd * GEMM(bf16(h[row_index[r]] * ln_w), W); h [Mh][1024] */
extern "C" int t3k_norm_gemm(const void* h, const void* ln_w, const void* w, int32_t M, int32_t N, float* out,
                             const int32_t* row_index, int32_t Mh) {
    if (!h || !ln_w || !w || !out || M <= 0 || N <= 0 || Mh <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    const int Npad = (N + 15) / 16 * 16;
    std::vector<uint16_t> folded((size_t)N * D), packed((size_t)Npad * D);
    fold_norm_weight((const uint16_t*)w, N, D, (const uint16_t*)ln_w, folded.data());      // what the engine does once at load time
    pack_weight(folded.data(), N, D, Npad, packed.data());
    DevBuf dh, dw, dout, dri;
    K_TRY(dh.from(h, (size_t)Mh * D * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2));
    K_TRY(dout.alloc((size_t)M * N * 4, true));
    if (row_index) K_TRY(dri.from(row_index, (size_t)M * 4));
    DevBuf drs; K_TRY(drs.alloc((size_t)M * 4));
    GemmArgs a{dh.as<uint16_t>(), dw.as<uint4>(), M, D, N, dout.p, N, 4, 1, row_index ? dri.as<int>() : nullptr, 0, drs.as<float>()};
    K_TRY(launch_gemm(a, EPI_F32, choose_mt(M, Npad / 16, 4, true), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* the qkv projection exactly as a step launches it: input RMSNorm folded, bf16 out [M][3072] */
extern "C" int t3k_qkv_gemm(const void* h, const void* ln_w, const void* w, int32_t M, void* out_bf16) {
    if (!h || !ln_w || !w || !out_bf16 || M <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    std::vector<uint16_t> folded((size_t)QKV * D), packed((size_t)QKV * D);
    fold_norm_weight((const uint16_t*)w, QKV, D, (const uint16_t*)ln_w, folded.data());
    pack_weight(folded.data(), QKV, D, QKV, packed.data());
    DevBuf dh, dw, dout, drs;
    K_TRY(dh.from(h, (size_t)M * D * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2)); K_TRY(dout.alloc((size_t)M * QKV * 2, true)); K_TRY(drs.alloc((size_t)M * 4));
    GemmArgs a{dh.as<uint16_t>(), dw.as<uint4>(), M, D, QKV, dout.p, QKV, 4, 1, nullptr, 0, drs.as<float>()};
    K_TRY(launch_gemm(a, EPI_BF16, choose_mt(M, QKV / 16, 4, true), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out_bf16, dout.p, (size_t)M * QKV * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* the speech head exactly as a step launches it: final RMSNorm folded, the sampled rows gathered through row_index, bf16 logits with
 * leading dimension 8208, the packed matrix padded to 516 n-tiles (tile groups may overhang the 8 194 columns) */
extern "C" int t3k_head_gemm(const void* h, const void* ln_w, const void* w, int32_t M, const int32_t* row_index, int32_t Mh, void* out_bf16) {
    if (!h || !ln_w || !w || !out_bf16 || !row_index || M <= 0 || Mh <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    std::vector<uint16_t> folded((size_t)V * D), packed((size_t)HEAD_TILES * 16 * D);
    fold_norm_weight((const uint16_t*)w, V, D, (const uint16_t*)ln_w, folded.data());
    pack_weight(folded.data(), V, D, HEAD_TILES * 16, packed.data());
    DevBuf dh, dw, dout, dri, drs;
    K_TRY(dh.from(h, (size_t)Mh * D * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2)); K_TRY(dout.alloc((size_t)M * VPAD * 2, true));
    K_TRY(dri.from(row_index, (size_t)M * 4)); K_TRY(drs.alloc((size_t)M * 4));
    // as the engine does: a decode-only step samples every row in row order, the gather is the identity and the head reads its rows directly
    bool identity = M == Mh;
    for (int i = 0; identity && i < M; ++i) identity = row_index[i] == i;
    GemmArgs a{dh.as<uint16_t>(), dw.as<uint4>(), M, D, V, dout.p, VPAD, 4, 1, identity ? nullptr : dri.as<int>(), HEAD_TILES, drs.as<float>()};
    K_TRY(launch_gemm(a, EPI_BF16, choose_mt(M, VPAD / 16, 4, true), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out_bf16, dout.p, (size_t)M * VPAD * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* residual epilogue of the o_proj / down_proj form: h [M][N] bf16 updated in place: h = bf16(h + bf16(x W^T)) */
extern "C" int t3k_gemm_resid(const void* x, const void* w, int32_t M, int32_t K, int32_t N, void* h_bf16) {
    if (!x || !w || !h_bf16 || M <= 0 || N <= 0 || N % 16 || K % 512) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    std::vector<uint16_t> packed((size_t)N * K);
    pack_weight((const uint16_t*)w, N, K, N, packed.data());
    DevBuf dx, dw, dh;
    K_TRY(dx.from(x, (size_t)M * K * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2)); K_TRY(dh.from(h_bf16, (size_t)M * N * 2));
    GemmArgs a{dx.as<uint16_t>(), dw.as<uint4>(), M, K, N, dh.p, N, 16, 0, nullptr};
    K_TRY(launch_gemm(a, EPI_RESID, choose_mt(M, N / 16, 16, false), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(h_bf16, dh.p, (size_t)M * N * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* gate/up form: out = bf16( bf16(silu(g)) * u ), g/u = bf16(rstd * GEMM(bf16(h*ln_w), Wg/Wu)) */
extern "C" int t3k_silu_mul_gemm(const void* h, const void* ln_w, const void* wg, const void* wu, int32_t M, int32_t Fd, void* out) {
    if (!h || !ln_w || !wg || !wu || !out || M <= 0 || Fd <= 0 || Fd % 16) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    gemm_refresh_switches();
    std::vector<uint16_t> fg((size_t)Fd * D), fu((size_t)Fd * D), packed((size_t)2 * Fd * D);
    fold_norm_weight((const uint16_t*)wg, Fd, D, (const uint16_t*)ln_w, fg.data());
    fold_norm_weight((const uint16_t*)wu, Fd, D, (const uint16_t*)ln_w, fu.data());
    pack_gate_up(fg.data(), fu.data(), Fd, D, packed.data());
    DevBuf dx, dw, dout;
    K_TRY(dx.from(h, (size_t)M * D * 2)); K_TRY(dw.from(packed.data(), packed.size() * 2)); K_TRY(dout.alloc((size_t)M * Fd * 2, true));
    DevBuf drs; K_TRY(drs.alloc((size_t)M * 4));
    GemmArgs a{dx.as<uint16_t>(), dw.as<uint4>(), M, D, Fd, dout.p, Fd, 4, 1, nullptr, 0, drs.as<float>()};
    K_TRY(launch_gemm(a, EPI_SILU, choose_mt(M, Fd / 16, 4, true), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)M * Fd * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}

// ---- the layer projections over MXFP8 weights (t3_gemm_mx8.hip): the arguments of their bf16 twins above; each folds the norm weight where its
// twin does, quantises and packs as t3_finalize_weights does under t3_set_weight_dtype = 1, and runs the kernel the engine runs
extern "C" int t3k_mxfp8_roundtrip(const void* w, void* y, int32_t rows, int32_t cols) {
    if (!w || !y || rows <= 0 || cols <= 0 || cols % 32) return T3_E_INVALID;
    mx8_roundtrip((const uint16_t*)w, (uint16_t*)y, rows, cols);
    return T3_OK;
}
static int mx8_run(const void* x, const std::vector<unsigned char>& packed, int rows, int M, int K, int N, int epi, void* out, bool out_is_input) {
    if (!have_device()) return T3_E_DEVICE;
    if (prepare_gemm_mx8() != hipSuccess) return T3_E_DEVICE;
    DevBuf dx, dw, dout;
    K_TRY(dx.from(x, (size_t)M * K * 2)); K_TRY(dw.from(packed.data(), packed.size()));
    if (out_is_input) K_TRY(dout.from(out, (size_t)M * N * 2)); else K_TRY(dout.alloc((size_t)M * N * 2, true));
    Mx8GemmArgs a{dx.as<uint16_t>(), dw.as<uint4>(), dw.as<unsigned char>() + (size_t)rows * K, M, K, N, dout.p, N};
    K_TRY(launch_gemm_mx8(a, epi, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)M * N * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}
extern "C" int t3k_qkv_gemm_mx8(const void* h, const void* ln_w, const void* w, int32_t M, void* out_bf16) {
    if (!h || !ln_w || !w || !out_bf16 || M <= 0) return T3_E_INVALID;
    std::vector<uint16_t> folded((size_t)QKV * D);
    std::vector<unsigned char> packed(mx8_packed_bytes(QKV, D));
    fold_norm_weight((const uint16_t*)w, QKV, D, (const uint16_t*)ln_w, folded.data());
    pack_weight_mx8(folded.data(), QKV, D, 8, packed.data());
    return mx8_run(h, packed, QKV, M, D, QKV, EPI_BF16, out_bf16, false);
}
extern "C" int t3k_gemm_resid_mx8(const void* x, const void* w, int32_t M, int32_t K, int32_t N, void* h_bf16) {
    if (!x || !w || !h_bf16 || M <= 0 || N <= 0 || N % 16 || (K != D && K != F)) return T3_E_INVALID;
    std::vector<unsigned char> packed(mx8_packed_bytes(N, K));
    pack_weight_mx8((const uint16_t*)w, N, K, K == D ? 2 : 8, packed.data());
    return mx8_run(x, packed, N, M, K, N, EPI_RESID, h_bf16, true);
}
extern "C" int t3k_silu_mul_gemm_mx8(const void* h, const void* ln_w, const void* wg, const void* wu, int32_t M, int32_t Fd, void* out) {
    if (!h || !ln_w || !wg || !wu || !out || M <= 0 || Fd <= 0 || Fd % 16) return T3_E_INVALID;
    std::vector<uint16_t> fg((size_t)Fd * D), fu((size_t)Fd * D);
    std::vector<unsigned char> packed(mx8_packed_bytes(2 * Fd, D));
    fold_norm_weight((const uint16_t*)wg, Fd, D, (const uint16_t*)ln_w, fg.data());
    fold_norm_weight((const uint16_t*)wu, Fd, D, (const uint16_t*)ln_w, fu.data());
    pack_gate_up_mx8(fg.data(), fu.data(), Fd, D, packed.data());
    return mx8_run(h, packed, 2 * Fd, M, D, Fd, EPI_SILU, out, false);
}

// fmt 1 / 4: the same call over an FP8 (E4M3) / MXFP4 pool -- byte pools, their own launchers; kv_out (nullable) [rows][2][1024] = the stored K / V read back
static int rope_attention_impl(const void* qkv, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                               int32_t n_streams, int32_t max_pos, void* out, int fmt, void* kv_out) {
    if (!qkv || !row_stream || !row_pos || !out || rows <= 0 || n_streams <= 0 || max_pos <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    for (int r = 0; r < rows; ++r)
        if (row_stream[r] < 0 || row_stream[r] >= n_streams || row_pos[r] < 0 || row_pos[r] >= max_pos) return T3_E_INVALID;
    const int max_blocks = (max_pos + KV_BLOCK - 1) / KV_BLOCK;
    // a deliberately scrambled block table, so that the test exercises the paging
    std::vector<int> table((size_t)n_streams * max_blocks);
    const int nb = n_streams * max_blocks;
    for (int i = 0; i < nb; ++i) table[i] = (int)(((long)i * 7919 + 13) % nb);
    {   // make it a permutation: 7919 is coprime with nb unless nb is a multiple of 7919
        std::vector<char> seen(nb, 0); bool ok = true;
        for (int i = 0; i < nb; ++i) { if (seen[table[i]]) ok = false; seen[table[i]] = 1; }
        if (!ok) for (int i = 0; i < nb; ++i) table[i] = nb - 1 - i;
    }
    std::vector<float> c((size_t)max_pos * 32), s((size_t)max_pos * 32);
    rope_tables(max_pos, c.data(), s.data());
    const int stride = row_stride_words(max_blocks);
    std::vector<int> recs((size_t)rows * stride, 0);
    for (int r = 0; r < rows; ++r) {
        int* rec = recs.data() + (size_t)r * stride;
        rec[0] = row_stream[r]; rec[1] = row_pos[r];
        for (int b = 0; b < max_blocks; ++b) rec[ROW_HDR + b] = table[(size_t)row_stream[r] * max_blocks + b];
    }
    DevBuf dqkv, drec, dc, ds, dq, dkv, dout;
    K_TRY(dqkv.from(qkv, (size_t)rows * QKV * 2)); K_TRY(drec.from(recs.data(), recs.size() * 4));
    K_TRY(dc.from(c.data(), c.size() * 4)); K_TRY(ds.from(s.data(), s.size() * 4));
    K_TRY(dq.alloc((size_t)rows * D * 2)); K_TRY(dkv.alloc((size_t)nb * kv_block_bytes(fmt), true)); K_TRY(dout.alloc((size_t)rows * D * 2, true));
    RopeArgs ra{dqkv.as<uint16_t>(), dq.as<uint16_t>(), dkv.as<uint16_t>(), drec.as<int>(), stride, dc.as<float>(), ds.as<float>(), rows};
    K_TRY(rope_kv_of(fmt, ra));
    AttnArgs aa{dq.as<uint16_t>(), dkv.as<uint16_t>(), drec.as<int>(), stride, dout.as<uint16_t>(), rows, (max_pos + CHUNK - 1) / CHUNK, nullptr, nullptr, nullptr, nullptr, 0, 0};     // every row through the 16-row tile schedule
    K_TRY(attention_of(fmt, aa));
    DevBuf dkvo;
    if (kv_out) { K_TRY(dkvo.alloc((size_t)rows * 2 * D * 2, true)); K_TRY(kv_gather_of(fmt, dkv.as<uint16_t>(), drec.as<int>(), stride, rows, dkvo.as<uint16_t>())); }
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)rows * D * 2, hipMemcpyDeviceToHost));
    if (kv_out) K_TRY(hipMemcpy(kv_out, dkvo.p, (size_t)rows * 2 * D * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}
extern "C" int t3k_rope_attention(const void* qkv, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                                  int32_t n_streams, int32_t max_pos, void* out) {
    return rope_attention_impl(qkv, row_stream, row_pos, rows, n_streams, max_pos, out, 0, nullptr);
}
extern "C" int t3k_rope_attention_fp8(const void* qkv, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                                      int32_t n_streams, int32_t max_pos, void* out, void* kv_out) {
    return rope_attention_impl(qkv, row_stream, row_pos, rows, n_streams, max_pos, out, 1, kv_out);
}
extern "C" int t3k_rope_attention_fp4(const void* qkv, const int32_t* row_stream, const int32_t* row_pos, int32_t rows,
                                      int32_t n_streams, int32_t max_pos, void* out, void* kv_out) {
    return rope_attention_impl(qkv, row_stream, row_pos, rows, n_streams, max_pos, out, 4, kv_out);
}

/* The alignment tap (t3_alignment.hip): every row goes into a scrambled paged pool through the prefill path (rope_kv), then ONE tap launch serves every
 * row (workgroup = row, frame = row) over the span [lo, hi) of its context. */
extern "C" int t3k_attention_probs(const void* qkv, const int32_t* row_stream, const int32_t* row_pos, int32_t rows, int32_t n_streams, int32_t max_pos,
                                   int32_t head, int32_t lo, int32_t hi, int32_t kv_dtype, float* out, void* q_rot, void* kv_out) {
    if (!qkv || !row_stream || !row_pos || !out || rows <= 0 || n_streams <= 0 || max_pos <= 0 || head < 0 || head >= H || lo < 0 || hi <= lo || hi > max_pos ||
        (kv_dtype != 0 && kv_dtype != 1 && kv_dtype != 4) || max_pos > 8192 /* the engine's own limit; the tap's LDS strip grows with it */) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    for (int r = 0; r < rows; ++r)
        if (row_stream[r] < 0 || row_stream[r] >= n_streams || row_pos[r] < 0 || row_pos[r] >= max_pos) return T3_E_INVALID;
    const int max_blocks = (max_pos + KV_BLOCK - 1) / KV_BLOCK, nb = n_streams * max_blocks, span = hi - lo;
    std::vector<int> table(nb);
    for (int i = 0; i < nb; ++i) table[i] = (int)(((long)i * 7919 + 13) % nb);
    {
        std::vector<char> seen(nb, 0); bool ok = true;
        for (int i = 0; i < nb; ++i) { if (seen[table[i]]) ok = false; seen[table[i]] = 1; }
        if (!ok) for (int i = 0; i < nb; ++i) table[i] = nb - 1 - i;
    }
    std::vector<float> c((size_t)max_pos * 32), s((size_t)max_pos * 32);
    rope_tables(max_pos, c.data(), s.data());
    const int stride = row_stride_words(max_blocks);
    std::vector<int> recs((size_t)rows * stride, 0);
    for (int r = 0; r < rows; ++r) {
        int* rec = recs.data() + (size_t)r * stride;
        rec[0] = row_stream[r]; rec[1] = row_pos[r]; rec[ROW_ALIGN_FRAME] = r; rec[ROW_ALIGN_NTEXT] = span;
        for (int b = 0; b < max_blocks; ++b) rec[ROW_HDR + b] = table[(size_t)row_stream[r] * max_blocks + b];
    }
    DevBuf dqkv, drec, dc, ds, dq, dkv, dout, dqr, dkvo;
    K_TRY(dqkv.from(qkv, (size_t)rows * QKV * 2)); K_TRY(drec.from(recs.data(), recs.size() * 4));
    K_TRY(dc.from(c.data(), c.size() * 4)); K_TRY(ds.from(s.data(), s.size() * 4));
    K_TRY(dq.alloc((size_t)rows * D * 2)); K_TRY(dkv.alloc((size_t)nb * kv_block_bytes(kv_dtype), true));
    K_TRY(dout.alloc((size_t)rows * span * 4, true)); K_TRY(dqr.alloc((size_t)rows * HD * 2, true));
    RopeArgs ra{dqkv.as<uint16_t>(), dq.as<uint16_t>(), dkv.as<uint16_t>(), drec.as<int>(), stride, dc.as<float>(), ds.as<float>(), rows};
    K_TRY(rope_kv_of(kv_dtype, ra));
    // frames_per_slot = 0: the destination row is the frame word alone, i.e. the row index
    AlignArgs aa{dqkv.as<uint16_t>(), dkv.p, drec.as<int>(), stride, nullptr, dc.as<float>(), ds.as<float>(), dout.as<float>(), rows, head, lo, (max_pos + CHUNK - 1) / CHUNK,
                 0, span, 0, 1, 1.0f, dqr.as<uint16_t>()};
    K_TRY(launch_alignment(aa, kv_dtype, nullptr));
    if (kv_out) { K_TRY(dkvo.alloc((size_t)rows * 2 * D * 2, true)); K_TRY(kv_gather_of(kv_dtype, dkv.as<uint16_t>(), drec.as<int>(), stride, rows, dkvo.as<uint16_t>())); }
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)rows * span * 4, hipMemcpyDeviceToHost));
    if (q_rot) K_TRY(hipMemcpy(q_rot, dqr.p, (size_t)rows * HD * 2, hipMemcpyDeviceToHost));
    if (kv_out) K_TRY(hipMemcpy(kv_out, dkvo.p, (size_t)rows * 2 * D * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* The FUSED decode attention exactly as a decode step launches it (attention_kernel<waves, nt, FUSE = true>: RoPE of q / k, paged
 * write of the newest K / V, attention over the paged context), `steps` consecutive launches of `rows` rows:
 *   - stream r (= row r) holds ctx[r] - 1 context tokens whose pre-RoPE qkv rows are ctx_qkv[content r % n_content][0 .. ctx[r] - 2]
 *     (written into a scrambled paged pool by rope_kv_kernel, the prefill path);
 *   - launch s processes, for every row r, the pre-RoPE row new_qkv[s][r] at position ctx[r] - 1 + s: launch s >= 1 therefore
 *     reads the K / V that launch s - 1 wrote through the fused path.
 * out [steps][rows][1024]; kv_new (nullable) [steps][rows][2][1024]: K (rotated) and V of the positions the launches wrote, read
 * back from the pool. */
static int decode_attention_impl(const void* ctx_qkv, int32_t n_content, int32_t content_rows, const void* new_qkv, const int32_t* ctx,
                                 int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out, void* kv_new, int fmt) {
    if (!ctx_qkv || !new_qkv || !ctx || !out || rows <= 0 || steps <= 0 || n_content <= 0 || content_rows <= 0 || max_pos <= 0 ||
        (waves != 0 && waves != 4 && waves != 8)) return T3_E_INVALID;
    for (int r = 0; r < rows; ++r)
        if (ctx[r] < 1 || ctx[r] - 1 > content_rows || ctx[r] - 1 + steps > max_pos) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    const int max_blocks = (max_pos + KV_BLOCK - 1) / KV_BLOCK, nb = rows * max_blocks;
    std::vector<int> table(nb);
    for (int i = 0; i < nb; ++i) table[i] = (int)(((long)i * 7919 + 13) % nb);
    {
        std::vector<char> seen(nb, 0); bool ok = true;
        for (int i = 0; i < nb; ++i) { if (seen[table[i]]) ok = false; seen[table[i]] = 1; }
        if (!ok) for (int i = 0; i < nb; ++i) table[i] = nb - 1 - i;
    }
    std::vector<float> c((size_t)max_pos * 32), s((size_t)max_pos * 32);
    rope_tables(max_pos, c.data(), s.data());
    const int stride = row_stride_words(max_blocks);
    DevBuf dctx, dnew, dc, ds, dq, dkv, dout, dkvn, drec_fill, drec;
    K_TRY(dctx.from(ctx_qkv, (size_t)n_content * content_rows * QKV * 2)); K_TRY(dnew.from(new_qkv, (size_t)steps * rows * QKV * 2));
    K_TRY(dc.from(c.data(), c.size() * 4)); K_TRY(ds.from(s.data(), s.size() * 4));
    K_TRY(dq.alloc((size_t)content_rows * D * 2));                     // rotated q of the fill rows: not used
    K_TRY(dkv.alloc((size_t)nb * kv_block_bytes(fmt), true)); K_TRY(dout.alloc((size_t)steps * rows * D * 2, true));
    K_TRY(dkvn.alloc((size_t)steps * rows * 2 * D * 2, true));
    // ---- context fill: one rope_kv launch per stream over its content's rows (positions 0 .. ctx[r] - 2)
    std::vector<int> recs((size_t)content_rows * stride);
    K_TRY(drec_fill.alloc(recs.size() * 4));
    for (int r = 0; r < rows; ++r) {
        const int n = ctx[r] - 1;
        if (n <= 0) continue;
        for (int p = 0; p < n; ++p) {
            int* rec = recs.data() + (size_t)p * stride;
            memset(rec, 0, (size_t)stride * 4);
            rec[0] = r; rec[1] = p;
            for (int b = 0; b < max_blocks; ++b) rec[ROW_HDR + b] = table[(size_t)r * max_blocks + b];
        }
        K_TRY(hipMemcpy(drec_fill.p, recs.data(), (size_t)n * stride * 4, hipMemcpyHostToDevice));
        RopeArgs ra{dctx.as<uint16_t>() + (size_t)(r % n_content) * content_rows * QKV, dq.as<uint16_t>(), dkv.as<uint16_t>(), drec_fill.as<int>(), stride,
                    dc.as<float>(), ds.as<float>(), n};
        K_TRY(rope_kv_of(fmt, ra));
        K_TRY(hipDeviceSynchronize());                                 // the record buffer is reused by the next stream
    }
    // ---- the decode launches
    std::vector<int> drecs((size_t)rows * stride, 0);
    K_TRY(drec.alloc(drecs.size() * 4));
    for (int st = 0; st < steps; ++st) {
        for (int r = 0; r < rows; ++r) {
            int* rec = drecs.data() + (size_t)r * stride;
            rec[0] = r; rec[1] = ctx[r] - 1 + st;
            for (int b = 0; b < max_blocks; ++b) rec[ROW_HDR + b] = table[(size_t)r * max_blocks + b];
        }
        K_TRY(hipMemcpy(drec.p, drecs.data(), drecs.size() * 4, hipMemcpyHostToDevice));
        AttnArgs aa{nullptr, dkv.as<uint16_t>(), drec.as<int>(), stride, dout.as<uint16_t>() + (size_t)st * rows * D, rows, (max_pos + CHUNK - 1) / CHUNK,
                    dnew.as<uint16_t>() + (size_t)st * rows * QKV, dkv.as<uint16_t>(), dc.as<float>(), ds.as<float>()};
        aa.force_waves = waves;
        K_TRY(attention_of(fmt, aa));
        K_TRY(kv_gather_of(fmt, dkv.as<uint16_t>(), drec.as<int>(), stride, rows, dkvn.as<uint16_t>() + (size_t)st * rows * 2 * D));
        K_TRY(hipDeviceSynchronize());
    }
    K_TRY(hipMemcpy(out, dout.p, (size_t)steps * rows * D * 2, hipMemcpyDeviceToHost));
    if (kv_new) K_TRY(hipMemcpy(kv_new, dkvn.p, (size_t)steps * rows * 2 * D * 2, hipMemcpyDeviceToHost));
    return T3_OK;
}
extern "C" int t3k_decode_attention(const void* ctx_qkv, int32_t n_content, int32_t content_rows, const void* new_qkv, const int32_t* ctx,
                                    int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out, void* kv_new) {
    return decode_attention_impl(ctx_qkv, n_content, content_rows, new_qkv, ctx, rows, steps, max_pos, waves, out, kv_new, 0);
}
extern "C" int t3k_decode_attention_fp8(const void* ctx_qkv, int32_t n_content, int32_t content_rows, const void* new_qkv, const int32_t* ctx,
                                        int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out, void* kv_new) {
    return decode_attention_impl(ctx_qkv, n_content, content_rows, new_qkv, ctx, rows, steps, max_pos, waves, out, kv_new, 1);
}
extern "C" int t3k_decode_attention_fp4(const void* ctx_qkv, int32_t n_content, int32_t content_rows, const void* new_qkv, const int32_t* ctx,
                                        int32_t rows, int32_t steps, int32_t max_pos, int32_t waves, void* out, void* kv_new) {
    return decode_attention_impl(ctx_qkv, n_content, content_rows, new_qkv, ctx, rows, steps, max_pos, waves, out, kv_new, 4);
}

static int sample_impl(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step,
                       int32_t* token_out, float* logits_out, uint8_t* keep_out, int32_t ctl = -1, const T3LogitProcessors* lp = nullptr);
extern "C" int t3k_sample(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step,
                          int32_t* token_out, float* logits_out) { return sample_impl(logits2, ldl, counts, sp, cfg, step, token_out, logits_out, nullptr); }
/* t3k_sample + the SUPPORT of the draw: keep_out [8194] = 1 where the masks (penalties -> /T -> min-p -> top-k -> top-p) leave the id drawable */
extern "C" int t3k_sample_support(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step,
                                  int32_t* token_out, uint8_t* keep_out) {
    if (!keep_out) return T3_E_INVALID;
    return sample_impl(logits2, ldl, counts, sp, cfg, step, token_out, nullptr, keep_out);
}
/* the sampler's guarded instantiation under one control word: the slot is marked guarded (alignment = 2) in the kernel's copy of sp */
extern "C" int t3k_sample_ctl(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step, int32_t ctl,
                              int32_t* token_out, float* logits_out) {
    if (ctl < GUARD_NONE || ctl > GUARD_FORCE || !sp || sp->stop_token < 0 || sp->stop_token >= V) return T3_E_INVALID;
    return sample_impl(logits2, ldl, counts, sp, cfg, step, token_out, logits_out, nullptr, ctl);
}
/* the sampler's third instantiation behind the build kernel: the record of slot 0 is made from *lp as the engine makes it at admission */
extern "C" int t3k_sample_proc(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp, float cfg, uint32_t step,
                               const T3LogitProcessors* lp, int32_t* token_out, float* logits_out, uint8_t* keep_out) {
    if (logitproc_check(lp)) return T3_E_INVALID;
    return sample_impl(logits2, ldl, counts, sp, cfg, step, token_out, logits_out, keep_out, -1, lp);
}
static int sample_impl(const void* logits2, int32_t ldl, uint16_t* counts, const T3Sampling* sp_in, float cfg, uint32_t step,
                       int32_t* token_out, float* logits_out, uint8_t* keep_out, int32_t ctl, const T3LogitProcessors* lp) {
    if (!logits2 || !counts || !sp_in || !token_out || ldl < V) return T3_E_INVALID;
    T3Sampling sp_copy = *sp_in; const T3Sampling* sp = &sp_copy;
    if (ctl >= 0) sp_copy.alignment = 2;
    if (!have_device()) return T3_E_DEVICE;
    std::vector<uint16_t> cpad(VPAD, 0);
    memcpy(cpad.data(), counts, V * 2);
    const int4 sel = make_int4(0, (int)step, 0, 0);
    DevBuf dl, dc, dsp, dsel, dtok, ddbg;
    K_TRY(dl.from(logits2, (size_t)2 * ldl * 2)); K_TRY(dc.from(cpad.data(), VPAD * 2)); K_TRY(dsp.from(sp, sizeof(T3Sampling)));
    K_TRY(dsel.from(&sel, sizeof(sel))); K_TRY(dtok.alloc(4, true)); K_TRY(ddbg.alloc((size_t)V * 4, true));
    SampleArgs sa{dl.as<uint16_t>(), ldl, dsel.as<int4>(), dc.as<uint16_t>(), dsp.as<T3Sampling>(), cfg, dtok.as<int>(), ddbg.as<float>(), 1};
    DevBuf dctl;
    if (ctl >= 0) { K_TRY(dctl.from(&ctl, 4)); sa.eos_ctl = dctl.as<int>(); }
    DevBuf dkeep;
    if (keep_out) { K_TRY(dkeep.alloc(V, true)); sa.dbg_keep = dkeep.as<unsigned char>(); }
    DevBuf dstage, drec, dproc;
    if (lp) {
        std::vector<int32_t> stage(PROC_STAGE_WORDS, 0); int32_t stops[PROC_MAX_STOP];
        logitproc_stage(lp, sp->stop_token, stage.data(), stops);
        K_TRY(dstage.from(stage.data(), stage.size() * 4)); K_TRY(drec.alloc((size_t)PROC_WORDS * 4, true)); K_TRY(dproc.alloc((size_t)V * 4, true));
        K_TRY(launch_logitproc_build(dstage.as<int32_t>(), drec.as<uint32_t>(), nullptr));
        sa.proc = drec.as<uint32_t>(); sa.dbg_proc = dproc.as<float>();
    }
    K_TRY(launch_sampler(sa, nullptr));
    K_TRY(hipDeviceSynchronize());
    if (keep_out) K_TRY(hipMemcpy(keep_out, dkeep.p, V, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(token_out, dtok.p, 4, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(cpad.data(), dc.p, VPAD * 2, hipMemcpyDeviceToHost));
    memcpy(counts, cpad.data(), V * 2);
    if (logits_out) K_TRY(hipMemcpy(logits_out, lp ? dproc.p : ddbg.p, (size_t)V * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* the log-probability kernel for one utterance: slot 0, step 0, its own k as the reserved maximum, the token as the sampler's output word */
extern "C" int t3k_logprobs(const void* logits2, int32_t ldl, float cfg, int32_t token, int32_t k, int32_t* rank, float* lp_tok,
                            int32_t* top_ids, float* top_lp) {
    if (!logits2 || !rank || !lp_tok || ldl < V || (ldl & 7) || token < 0 || token >= V || k < 0 || k > T3_MAX_LOGPROBS || (k > 0 && (!top_ids || !top_lp)))
        return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    const int4 sel = make_int4(0, 0, 0, 0);
    std::vector<int32_t> rec((size_t)2 * (k + 1), 0);
    DevBuf dl, dsel, dtok, dk, drec;
    K_TRY(dl.from(logits2, (size_t)2 * ldl * 2)); K_TRY(dsel.from(&sel, sizeof(sel))); K_TRY(dtok.from(&token, 4)); K_TRY(dk.from(&k, 4));
    K_TRY(drec.alloc(rec.size() * 4, true));
    LogprobArgs la{dl.as<uint16_t>(), ldl, dsel.as<int4>(), dtok.as<int>(), dk.as<int>(), cfg, drec.as<int>(), 1, k, 1};
    K_TRY(launch_logprobs(la, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(rec.data(), drec.p, rec.size() * 4, hipMemcpyDeviceToHost));
    *rank = rec[0]; memcpy(lp_tok, &rec[1], 4);
    for (int i = 0; i < k; ++i) { top_ids[i] = rec[2 + 2 * i]; memcpy(top_lp + i, &rec[3 + 2 * i], 4); }
    return T3_OK;
}

/* its processed instantiation for one utterance: slot 0, token `step`.  counts = what the step's sampler USED; the device copy gets the drawn id's
 * increment as sampler_kernel's finish() leaves it, because that is the state the kernel meets in the engine.  The record of *lp is built as at
 * admission; ctl >= 0 marks the slot guarded in the kernel's copy of sp, as t3k_sample_ctl does. */
extern "C" int t3k_logprobs_processed(const void* logits2, int32_t ldl, float cfg, const uint16_t* counts, const T3Sampling* sp_in, const T3LogitProcessors* lp,
                                      int32_t ctl, uint32_t step, int32_t token, int32_t k, int32_t* rank, float* lp_tok, int32_t* top_ids, float* top_lp) {
    if (!logits2 || !counts || !sp_in || !rank || !lp_tok || ldl < V || (ldl & 7) || token < 0 || token >= V || k < 0 || k > T3_MAX_LOGPROBS ||
        (k > 0 && (!top_ids || !top_lp)) || ctl < -1 || ctl > GUARD_FORCE || step >= 8192u /* the engine's largest max_model_len */)
        return T3_E_INVALID;
    if (ctl >= 0 && (sp_in->stop_token < 0 || sp_in->stop_token >= V)) return T3_E_INVALID;
    if (lp && logitproc_check(lp)) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    T3Sampling sp = *sp_in;
    if (ctl >= 0) sp.alignment = 2;
    std::vector<uint16_t> cpad(VPAD, 0);
    memcpy(cpad.data(), counts, V * 2);
    if (cpad[token] < 65535) ++cpad[token];
    const int4 sel = make_int4(0, (int)step, 0, 0);
    const size_t recw = (size_t)2 * (k + 1);      // the kernel writes record `step` of step + 1
    std::vector<int32_t> rec(recw, 0);
    DevBuf dl, dc, dsp, dsel, dtok, dk, drec, dctl, dstage, dproc;
    K_TRY(dl.from(logits2, (size_t)2 * ldl * 2)); K_TRY(dc.from(cpad.data(), VPAD * 2)); K_TRY(dsp.from(&sp, sizeof(sp)));
    K_TRY(dsel.from(&sel, sizeof(sel))); K_TRY(dtok.from(&token, 4)); K_TRY(dk.from(&k, 4)); K_TRY(drec.alloc((size_t)(step + 1) * recw * 4, true));
    LogprobArgs la{dl.as<uint16_t>(), ldl, dsel.as<int4>(), dtok.as<int>(), dk.as<int>(), cfg, drec.as<int>(), (int)step + 1, k, 1};
    la.counts = dc.as<uint16_t>(); la.sp = dsp.as<T3Sampling>(); la.mode = 1;
    if (ctl >= 0) { K_TRY(dctl.from(&ctl, 4)); la.eos_ctl = dctl.as<int>(); }
    if (lp) {
        std::vector<int32_t> stage(PROC_STAGE_WORDS, 0); int32_t stops[PROC_MAX_STOP];
        logitproc_stage(lp, sp.stop_token, stage.data(), stops);
        K_TRY(dstage.from(stage.data(), stage.size() * 4)); K_TRY(dproc.alloc((size_t)PROC_WORDS * 4, true));
        K_TRY(launch_logitproc_build(dstage.as<int32_t>(), dproc.as<uint32_t>(), nullptr));
        la.proc = dproc.as<uint32_t>();
    }
    K_TRY(launch_logprobs(la, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(rec.data(), drec.as<int>() + (size_t)step * recw, recw * 4, hipMemcpyDeviceToHost));
    *rank = rec[0]; memcpy(lp_tok, &rec[1], 4);
    for (int i = 0; i < k; ++i) { top_ids[i] = rec[2 + 2 * i]; memcpy(top_lp + i, &rec[3 + 2 * i], 4); }
    return T3_OK;
}

/* the hand-off kernel on host buffers: ids [n] speech-space -> out [ld] (padded with 0), *len */
extern "C" int t3k_handoff(const int32_t* ids, int32_t n, int32_t text_token_count, int32_t flags, int32_t* out, int32_t ld, int32_t* len) {
    if ((!ids && n > 0) || !out || !len || n < 0 || ld <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    DevBuf dids, ditem, dout, dlen;
    K_TRY(dids.from(ids, (size_t)n * 4)); K_TRY(dout.alloc((size_t)ld * 4, true)); K_TRY(dlen.alloc(4, true));
    const HandoffItem item{dids.as<int>(), n, text_token_count, 0};
    K_TRY(ditem.from(&item, sizeof(item)));
    K_TRY(launch_handoff(ditem.as<HandoffItem>(), 1, flags, dout.as<int>(), ld, dlen.as<int>(), nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(out, dout.p, (size_t)ld * 4, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(len, dlen.p, 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

extern "C" int t3k_fp8_roundtrip(const float* x, float* y, int32_t n) {
    if (!x || !y || n <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    DevBuf dx, dy;
    K_TRY(dx.from(x, (size_t)n * 4)); K_TRY(dy.alloc((size_t)n * 4));
    K_TRY(launch_fp8_roundtrip(dx.as<float>(), dy.as<float>(), n, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(y, dy.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

extern "C" int t3k_fp4_roundtrip(const float* x, float* y, int32_t n) {
    if (!x || !y || n <= 0 || n % 32) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    DevBuf dx, dy;
    K_TRY(dx.from(x, (size_t)n * 4)); K_TRY(dy.alloc((size_t)n * 4));
    K_TRY(launch_fp4_roundtrip(dx.as<float>(), dy.as<float>(), n, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(y, dy.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

extern "C" int t3k_expf(const float* x, float* y, int32_t n) {
    if (!x || !y || n <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    DevBuf dx, dy;
    K_TRY(dx.from(x, (size_t)n * 4)); K_TRY(dy.alloc((size_t)n * 4));
    K_TRY(launch_expf(dx.as<float>(), dy.as<float>(), n, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(y, dy.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

/* The guard kernel (t3_guard.hip) frame by frame over a host matrix: slot 0, frame k = launch k, the ids as the sampler's history. */
extern "C" int t3k_alignment_guard(const float* A, int32_t n_frames, int32_t n_text, int32_t ld, const int32_t* tok, const T3GuardParams* params,
                                   int32_t* ctl_out, T3GuardState* final_state) {
    if (!A || !tok || !params || !ctl_out || !final_state || n_frames <= 0 || n_text <= 0 || ld < n_text || (ld & 3)) return T3_E_INVALID;
    for (int k = 0; k < n_frames; ++k) if (tok[k] < 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    const int stride = row_stride_words(1);
    std::vector<int> recs((size_t)n_frames * stride, 0);
    std::vector<int4> sel(n_frames);
    for (int k = 0; k < n_frames; ++k) {
        recs[(size_t)k * stride + ROW_ALIGN_FRAME] = k; recs[(size_t)k * stride + ROW_ALIGN_NTEXT] = n_text;
        sel[k] = make_int4(0, k, 0, 0);
    }
    T3Sampling sp{}; sp.alignment = 2; sp.stop_token = -1;      // no id ends the utterance here
    DevBuf dA, dtok, drec, dsel, dsp, dstate, dctl;
    K_TRY(dA.from(A, (size_t)n_frames * ld * 4)); K_TRY(dtok.from(tok, (size_t)n_frames * 4)); K_TRY(drec.from(recs.data(), recs.size() * 4));
    K_TRY(dsel.from(sel.data(), sel.size() * sizeof(int4))); K_TRY(dsp.from(&sp, sizeof(sp)));
    K_TRY(dstate.alloc(GUARD_STATE_WORDS * 4)); K_TRY(dctl.alloc((size_t)n_frames * 4, true));
    K_TRY(launch_guard_reset(dstate.as<int>(), dctl.as<int>(), 0, nullptr));
    for (int k = 0; k < n_frames; ++k) {      // launch k: its record, its sel entry, its own control word
        GuardArgs ga{dA.as<float>(), n_frames, ld, drec.as<int>() + (size_t)k * stride, stride, nullptr, dsel.as<int4>() + k, dsp.as<T3Sampling>(),
                     dtok.as<int>(), n_frames, dstate.as<int>(), dctl.as<int>() + k, 1, *params};
        K_TRY(launch_guard(ga, nullptr));
    }
    K_TRY(hipDeviceSynchronize());
    int words[GUARD_STATE_WORDS];
    K_TRY(hipMemcpy(words, dstate.p, sizeof(words), hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(ctl_out, dctl.p, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    guard_unpack_state(words, final_state);
    return T3_OK;
}

/* The path kernel (t3_align_path.hip) on one host matrix: the launch the engine makes for a finished request, with a workspace of its own. */
extern "C" int t3k_align_path(const float* A, int32_t n_frames, int32_t n_text, int32_t ld, int32_t* path, int32_t* start, int32_t* end,
                              int32_t* last, int32_t* score) {
    if (!A || !path || !start || !end || !last || !score || n_frames <= 0 || n_frames > ALIGN_PATH_MAX_FRAMES || n_text <= 0 ||
        n_text > ALIGN_PATH_MAX_TEXT || ld < n_text) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    const int ns = (n_text + 63) / 64;
    DevBuf dA, dbp, dpath, dse, dres, ditem;
    K_TRY(dA.from(A, (size_t)n_frames * ld * 4)); K_TRY(dbp.alloc((size_t)n_frames * ns * 8, true)); K_TRY(dpath.alloc((size_t)n_frames * 4, true));
    K_TRY(dse.alloc((size_t)2 * n_text * 4)); K_TRY(dres.alloc(8, true));
    const AlignPathItem item{dA.as<float>(), n_frames, n_text, ld, 0, dbp.as<unsigned long long>(), dpath.as<int>(), dse.as<int>(), dse.as<int>() + n_text, dres.as<int>()};
    K_TRY(ditem.from(&item, sizeof(item)));
    K_TRY(launch_align_path(ditem.as<AlignPathItem>(), 1, n_text, n_text, nullptr));
    K_TRY(hipDeviceSynchronize());
    int res[2];
    K_TRY(hipMemcpy(path, dpath.p, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(start, dse.p, (size_t)n_text * 4, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(end, dse.as<int>() + n_text, (size_t)n_text * 4, hipMemcpyDeviceToHost));
    K_TRY(hipMemcpy(res, dres.p, 8, hipMemcpyDeviceToHost));
    *last = res[0]; *score = res[1];
    return T3_OK;
}

/* the cell score of the path kernel alone: w[i] = round(1024 log2 a'[i]) */
extern "C" int t3k_align_scores(const float* a, int32_t* w, int32_t n) {
    if (!a || !w || n <= 0) return T3_E_INVALID;
    if (!have_device()) return T3_E_DEVICE;
    DevBuf da, dw;
    K_TRY(da.from(a, (size_t)n * 4)); K_TRY(dw.alloc((size_t)n * 4));
    K_TRY(launch_align_scores(da.as<float>(), dw.as<int>(), n, nullptr));
    K_TRY(hipDeviceSynchronize());
    K_TRY(hipMemcpy(w, dw.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return T3_OK;
}

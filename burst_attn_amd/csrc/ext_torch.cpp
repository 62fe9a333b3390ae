// Torch bindings for the BurstAttention gfx950 kernels.
//
// Thin layer only: shape/stride checks, output allocation, current-stream
// plumbing.  All compute goes through the C ABI in
// include/burst_attn_hip.h (see that header for the reference call sites
// each entry point replaces).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "../../include/burst_attn_hip.h"
#include "probes.h"

namespace {

int dtype_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kHalf) return BAHIP_F16;
  if (t.scalar_type() == at::kBFloat16) return BAHIP_BF16;
  TORCH_CHECK(false, "burst_attn: expected fp16 or bf16, got ", t.scalar_type());
  return -1;
}

void check_qkv(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.dim() == 4, name, " must be [B,S,N,D]");
  TORCH_CHECK(t.stride(3) == 1, name, " head_dim must be contiguous");
  TORCH_CHECK(t.stride(1) % 8 == 0, name,
              " seq stride must be a multiple of 8 elements (16B alignment)");
  TORCH_CHECK(t.stride(2) % 8 == 0, name,
              " head stride must be a multiple of 8 elements");
}

// {batch, seq, head} element strides of a [B,S,N,D] tensor, as the C ABI
// takes them
struct Strides3 {
  int64_t s[3];
  explicit Strides3(const at::Tensor& t)
      : s{t.stride(0), t.stride(1), t.stride(2)} {}
  operator const int64_t*() const { return s; }
};

// per-tensor layout plus cross-tensor consistency vs q: batch/head_dim
// agree, k/v heads and seqlens agree, q heads are a multiple of the k/v
// heads (grouped-query: q head h attends kv head h / G), dtypes are equal
// — a mismatch must raise here, not read out of bounds on device.
void check_qkv3(const at::Tensor& q, const at::Tensor& k,
                const at::Tensor& v) {
  check_qkv(q, "q");
  check_qkv(k, "k");
  check_qkv(v, "v");
  TORCH_CHECK(k.size(0) == q.size(0) && v.size(0) == q.size(0),
              "batch mismatch");
  TORCH_CHECK(v.size(2) == k.size(2), "k/v heads mismatch (", k.size(2),
              " vs ", v.size(2), ")");
  TORCH_CHECK(k.size(2) >= 1 && q.size(2) % k.size(2) == 0,
              "heads mismatch: q heads N=", q.size(2),
              " must be a multiple of kv heads Nk=", k.size(2));
  TORCH_CHECK(k.size(3) == q.size(3) && v.size(3) == q.size(3),
              "head_dim mismatch");
  TORCH_CHECK(v.size(1) == k.size(1), "k/v seqlen mismatch");
  TORCH_CHECK(q.scalar_type() == k.scalar_type() &&
                  q.scalar_type() == v.scalar_type(),
              "q/k/v dtype mismatch");
}

#define BA_CALL(expr)                                                      \
  do {                                                                     \
    int rc_ = (expr);                                                      \
    TORCH_CHECK(rc_ == 0, "burst_attn HIP kernel failed (rc=", rc_, "): ", \
                bahip_last_error());                                       \
  } while (0)

// Workspace for the V^T image of this call, or an undefined tensor where
// the knobs and the auto rule keep the in-kernel transpose.  Allocated per
// call on the current stream and never cached: the ring hands the same k/v
// buffers in with new contents every round.
at::Tensor fwd_workspace(const at::Tensor& q, const at::Tensor& k) {
  const int64_t bytes = bahip_attn_fwd_workspace_bytes(
      q.size(0), q.size(1), k.size(1), q.size(2), k.size(2), q.size(3));
  if (bytes <= 0) return at::Tensor();
  return at::empty({bytes}, q.options().dtype(at::kByte));
}

// Segment ids of a call: both or neither; int32 [B, Sq] / [B, Sk] with a
// contiguous seq dim, on q's device.  A given pair comes with the pre-pass
// workspace, allocated per call on the current stream like the V^T image's.
struct SegIds {
  const int32_t *q = nullptr, *kv = nullptr;
  int64_t q_sb = 0, kv_sb = 0;
  at::Tensor ws;
  void* ws_ptr() const { return ws.defined() ? ws.data_ptr() : nullptr; }
  int64_t ws_bytes() const { return ws.defined() ? ws.numel() : 0; }
};

void check_seg(const at::Tensor& s, const at::Tensor& q, int64_t rows,
               const char* name) {
  TORCH_CHECK(s.scalar_type() == at::kInt, name, " must be int32, got ",
              s.scalar_type());
  TORCH_CHECK(s.device() == q.device(), name, " must be on q's device");
  TORCH_CHECK(s.dim() == 2 && s.size(0) == q.size(0) && s.size(1) == rows,
              name, " must be [B, S] = [", q.size(0), ", ", rows, "], got ",
              s.sizes());
  TORCH_CHECK(s.stride(1) == 1 || rows == 1, name,
              " seq dim must be contiguous");
}

SegIds seg_ids(const c10::optional<at::Tensor>& q_seg,
               const c10::optional<at::Tensor>& kv_seg, const at::Tensor& q,
               const at::Tensor& k) {
  SegIds s;
  TORCH_CHECK(q_seg.has_value() == kv_seg.has_value(),
              "q_seg and kv_seg must be given together");
  if (!q_seg.has_value()) return s;
  check_seg(*q_seg, q, q.size(1), "q_seg");
  check_seg(*kv_seg, q, k.size(1), "kv_seg");
  s.q = q_seg->data_ptr<int32_t>();
  s.kv = kv_seg->data_ptr<int32_t>();
  s.q_sb = q_seg->stride(0);
  s.kv_sb = kv_seg->stride(0);
  s.ws = at::empty(
      {bahip_attn_seg_workspace_bytes(q.size(0), q.size(1), k.size(1))},
      q.options().dtype(at::kByte));
  return s;
}

// The band of a call: band_lo and band_hi together or not at all, and never
// together with segment ids (that combination has no kernel form yet).
bool band_given(const c10::optional<int64_t>& band_lo,
                const c10::optional<int64_t>& band_hi, const SegIds& seg) {
  TORCH_CHECK(band_lo.has_value() == band_hi.has_value(),
              "band_lo and band_hi must be given together");
  TORCH_CHECK(!(band_lo.has_value() && seg.q),
              "band_lo/band_hi and q_seg/kv_seg are not supported together "
              "yet");
  return band_lo.has_value();
}

// The pre-pass alone on [B, Sq] / [B, Sk] ids: the workspace as int32
// words (layout: bahip_attn_seg_prepass).  For tests and measurements.
at::Tensor attn_seg_prepass(const at::Tensor& q_seg, const at::Tensor& kv_seg) {
  TORCH_CHECK(q_seg.is_cuda() && kv_seg.is_cuda() && q_seg.dim() == 2 &&
                  kv_seg.dim() == 2 && q_seg.size(0) == kv_seg.size(0) &&
                  q_seg.scalar_type() == at::kInt &&
                  kv_seg.scalar_type() == at::kInt &&
                  (q_seg.stride(1) == 1 || q_seg.size(1) == 1) &&
                  (kv_seg.stride(1) == 1 || kv_seg.size(1) == 1),
              "segment ids must be int32 [B, S] GPU tensors, seq contiguous");
  const auto B = q_seg.size(0), Sq = q_seg.size(1), Sk = kv_seg.size(1);
  auto ws = at::empty({bahip_attn_seg_workspace_bytes(B, Sq, Sk) / 4},
                      q_seg.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_seg_prepass(q_seg.data_ptr<int32_t>(),
                                 kv_seg.data_ptr<int32_t>(), q_seg.stride(0),
                                 kv_seg.stride(0), B, Sq, Sk, ws.data_ptr(),
                                 ws.numel() * 4, stream));
  return ws;
}

std::vector<at::Tensor> attn_fwd(const at::Tensor& q, const at::Tensor& k,
                                 const at::Tensor& v, double softmax_scale,
                                 bool causal,
                                 const c10::optional<at::Tensor>& q_seg,
                                 const c10::optional<at::Tensor>& kv_seg,
                                 const c10::optional<int64_t>& band_lo,
                                 const c10::optional<int64_t>& band_hi) {
  check_qkv3(q, k, v);
  const auto B = q.size(0), Sq = q.size(1), N = q.size(2), D = q.size(3);
  const auto Sk = k.size(1);
  const SegIds seg = seg_ids(q_seg, kv_seg, q, k);
  auto o = at::empty({B, Sq, N, D}, q.options().dtype(at::kFloat));
  auto lse = at::empty({B, N, Sq}, q.options().dtype(at::kFloat));
  if (band_given(band_lo, band_hi, seg)) {
    BA_CALL(bahip_attn_fwd_band(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr<float>(),
        lse.data_ptr<float>(), B, Sq, Sk, N, k.size(2), D, Strides3(q),
        Strides3(k), Strides3(v), (float)softmax_scale, causal ? 1 : 0,
        dtype_code(q), *band_lo, *band_hi,
        at::hip::getCurrentHIPStream().stream()));
    return {o, lse};
  }
  // with ids the forward transposes V in the kernel: no image workspace
  auto ws = seg.q ? at::Tensor() : fwd_workspace(q, k);
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_fwd_seg(
      q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr<float>(),
      lse.data_ptr<float>(), B, Sq, Sk, N, k.size(2), D, Strides3(q),
      Strides3(k), Strides3(v), (float)softmax_scale, causal ? 1 : 0,
      dtype_code(q), ws.defined() ? ws.data_ptr() : nullptr,
      ws.defined() ? ws.numel() : 0, seg.q, seg.kv, seg.q_sb, seg.kv_sb,
      seg.ws_ptr(), seg.ws_bytes(), stream));
  return {o, lse};
}

// The V^T image of v ([B, Sk, Nk, D], strided) as a [B, Nk, T, D, 64]
// tensor, T = ceil(Sk / 64): what the forward's pre-pass writes.
at::Tensor attn_vt_image(const at::Tensor& v, c10::optional<at::Tensor> out) {
  check_qkv(v, "v");
  const auto B = v.size(0), Sk = v.size(1), Nk = v.size(2), D = v.size(3);
  const int64_t T = (Sk + 63) / 64;
  // `out` is either the image tensor itself or a flat workspace of v's
  // dtype, handed to the C entry with its true size: whether it is large
  // enough is the launcher's check (BAHIP_ERR_WORKSPACE), not this layer's.
  at::Tensor img;
  if (out.has_value()) {
    img = *out;
    TORCH_CHECK(img.is_cuda() && img.scalar_type() == v.scalar_type() &&
                    img.is_contiguous() &&
                    (img.dim() == 1 ||
                     img.sizes() == at::IntArrayRef({B, Nk, T, D, 64})),
                "image out must be contiguous, of v's dtype, and either "
                "[B,Nk,ceil(Sk/64),D,64] or a flat workspace");
  } else {
    img = at::empty({B, Nk, T, D, 64}, v.options());
  }
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_vt_image(v.data_ptr(), img.data_ptr(),
                              img.numel() * img.element_size(), B, Sk, Nk, D,
                              Strides3(v), dtype_code(v), stream));
  if (img.dim() == 1) return img.narrow(0, 0, B * Nk * T * D * 64)
                          .view({B, Nk, T, D, 64});
  return img;
}

// Checks and stride extraction shared by attn_fwd_accum (asm_fn null: the
// in-binary kernel the BA_FWD_* knobs select) and attn_fwd_accum_asm
// (asm_fn: the hipModule-loaded kernel).
void fwd_accum_call(void* asm_fn, const at::Tensor& q, const at::Tensor& k,
                    const at::Tensor& v, double softmax_scale, bool causal,
                    at::Tensor& acc, at::Tensor& m, at::Tensor& l,
                    bool carry_in,
                    const c10::optional<at::Tensor>& q_seg = c10::nullopt,
                    const c10::optional<at::Tensor>& kv_seg = c10::nullopt,
                    const c10::optional<int64_t>& band_lo = c10::nullopt,
                    const c10::optional<int64_t>& band_hi = c10::nullopt) {
  check_qkv3(q, k, v);
  const auto B = q.size(0), Sq = q.size(1), N = q.size(2), D = q.size(3);
  const auto Sk = k.size(1);
  const SegIds seg = seg_ids(q_seg, kv_seg, q, k);
  TORCH_CHECK(acc.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat
                  && l.scalar_type() == at::kFloat, "state must be fp32");
  TORCH_CHECK(acc.size(1) == Sq && m.size(2) == Sq && l.size(2) == Sq,
              "state rows must match q rows");
  TORCH_CHECK(acc.stride(3) == 1 && m.stride(2) == 1 && l.stride(2) == 1,
              "state innermost dims must be contiguous");
  int64_t mls[2] = {m.stride(0), m.stride(1)};
  TORCH_CHECK(l.stride(0) == mls[0] && l.stride(1) == mls[1],
              "m/l stride mismatch");
  if (band_given(band_lo, band_hi, seg)) {
    BA_CALL(bahip_attn_fwd_accum_band(
        nullptr, q.data_ptr(), k.data_ptr(), v.data_ptr(), B, Sq, Sk, N,
        k.size(2), D, Strides3(q), Strides3(k), Strides3(v),
        (float)softmax_scale, causal ? 1 : 0, dtype_code(q),
        acc.data_ptr<float>(), m.data_ptr<float>(), l.data_ptr<float>(),
        Strides3(acc), mls, carry_in ? 1 : 0, *band_lo, *band_hi,
        at::hip::getCurrentHIPStream().stream()));
    return;
  }
  // the module kernel and the segment form transpose V themselves: no
  // image workspace
  auto ws = (asm_fn || seg.q) ? at::Tensor() : fwd_workspace(q, k);
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_fwd_accum_seg(
      asm_fn, q.data_ptr(), k.data_ptr(), v.data_ptr(), B, Sq, Sk, N,
      k.size(2), D, Strides3(q), Strides3(k), Strides3(v), (float)softmax_scale,
      causal ? 1 : 0, dtype_code(q), acc.data_ptr<float>(),
      m.data_ptr<float>(), l.data_ptr<float>(), Strides3(acc), mls,
      carry_in ? 1 : 0, ws.defined() ? ws.data_ptr() : nullptr,
      ws.defined() ? ws.numel() : 0, seg.q, seg.kv, seg.q_sb, seg.kv_sb,
      seg.ws_ptr(), seg.ws_bytes(), stream));
}

void attn_fwd_accum(const at::Tensor& q, const at::Tensor& k,
                    const at::Tensor& v, double softmax_scale, bool causal,
                    at::Tensor& acc, at::Tensor& m, at::Tensor& l,
                    bool carry_in, const c10::optional<at::Tensor>& q_seg,
                    const c10::optional<at::Tensor>& kv_seg,
                    const c10::optional<int64_t>& band_lo,
                    const c10::optional<int64_t>& band_hi) {
  fwd_accum_call(nullptr, q, k, v, softmax_scale, causal, acc, m, l, carry_in,
                 q_seg, kv_seg, band_lo, band_hi);
}

// The empty carry-in state ("no key seen yet") written into acc [B,S,N,D],
// m and l [B,N,S] (fp32, strided views allowed as in attn_fwd_accum).
void attn_fwd_state_init(at::Tensor& acc, at::Tensor& m, at::Tensor& l) {
  TORCH_CHECK(acc.is_cuda() && m.is_cuda() && l.is_cuda() && acc.dim() == 4 &&
                  m.dim() == 3 && l.dim() == 3,
              "state must be GPU tensors acc [B,S,N,D], m/l [B,N,S]");
  TORCH_CHECK(acc.scalar_type() == at::kFloat && m.scalar_type() == at::kFloat
                  && l.scalar_type() == at::kFloat, "state must be fp32");
  const auto B = acc.size(0), S = acc.size(1), N = acc.size(2), D = acc.size(3);
  TORCH_CHECK(m.sizes() == at::IntArrayRef({B, N, S}) && l.sizes() == m.sizes(),
              "m/l must be [B,N,S] of acc's [B,S,N,D]");
  TORCH_CHECK(acc.stride(3) == 1 && m.stride(2) == 1 && l.stride(2) == 1,
              "state innermost dims must be contiguous");
  int64_t mls[2] = {m.stride(0), m.stride(1)};
  TORCH_CHECK(l.stride(0) == mls[0] && l.stride(1) == mls[1],
              "m/l stride mismatch");
  BA_CALL(bahip_attn_fwd_state_init(
      acc.data_ptr<float>(), m.data_ptr<float>(), l.data_ptr<float>(), B, S, N,
      D, Strides3(acc), mls, at::hip::getCurrentHIPStream().stream()));
}

std::vector<at::Tensor> attn_fwd_finalize(const at::Tensor& acc,
                                          const at::Tensor& m,
                                          const at::Tensor& l,
                                          at::ScalarType out_dtype) {
  TORCH_CHECK(acc.is_contiguous() && m.is_contiguous() && l.is_contiguous());
  const auto B = acc.size(0), S = acc.size(1), N = acc.size(2), D = acc.size(3);
  auto o = at::empty({B, S, N, D}, acc.options().dtype(out_dtype));
  auto lse = at::empty({B, N, S}, acc.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_fwd_finalize(
      acc.data_ptr<float>(), m.data_ptr<float>(), l.data_ptr<float>(),
      o.data_ptr(), lse.data_ptr<float>(), B, S, N, D,
      out_dtype == at::kHalf ? BAHIP_F16 : BAHIP_BF16, stream));
  return {o, lse};
}

at::Tensor attn_bwd_preprocess(const at::Tensor& o, const at::Tensor& dout,
                               c10::optional<at::Tensor> out) {
  check_qkv(o, "o");
  check_qkv(dout, "dout");
  const auto B = o.size(0), S = o.size(1), N = o.size(2), D = o.size(3);
  TORCH_CHECK(dout.sizes() == o.sizes(), "o/dout shape mismatch");
  at::Tensor delta;
  if (out.has_value()) {
    delta = *out;
    TORCH_CHECK(delta.scalar_type() == at::kFloat && delta.is_contiguous() &&
                    delta.sizes() == at::IntArrayRef({B, N, S}),
                "preprocess out must be contiguous fp32 [B,N,S]");
  } else {
    delta = at::empty({B, N, S}, o.options().dtype(at::kFloat));
  }
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_attn_bwd_preprocess(o.data_ptr(), dout.data_ptr(),
                                    delta.data_ptr<float>(), B, S, N, D,
                                    Strides3(o), Strides3(dout), dtype_code(o),
                                    dtype_code(dout), stream));
  return delta;
}

void check_grad_out(const at::Tensor& g, const at::Tensor& like,
                    const char* name) {
  TORCH_CHECK(g.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(g.scalar_type() == at::kFloat, name,
              " accumulator must be fp32");
  TORCH_CHECK(g.dim() == 4, name, " must be [B,S,N,D]");
  TORCH_CHECK(g.stride(3) == 1, name, " head_dim must be contiguous");
  TORCH_CHECK(g.sizes() == like.sizes(), name, " shape mismatch");
}

// in-place accumulate: dq/dk/dv (fp32, strided views allowed) += tile
// contribution.  The ring layer's round accumulation happens HERE, not
// in python adds (reference burst_attn_interface.py:379-390).
void attn_bwd_accum(const at::Tensor& dout, const at::Tensor& q,
                    const at::Tensor& k, const at::Tensor& v,
                    const at::Tensor& delta, const at::Tensor& lse,
                    double softmax_scale, bool causal, bool deterministic,
                    at::Tensor& dq, at::Tensor& dk, at::Tensor& dv,
                    const c10::optional<at::Tensor>& q_seg,
                    const c10::optional<at::Tensor>& kv_seg,
                    const c10::optional<int64_t>& band_lo,
                    const c10::optional<int64_t>& band_hi) {
  check_qkv(dout, "dout");
  check_qkv3(q, k, v);
  const auto B = q.size(0), Sq = q.size(1), N = q.size(2), D = q.size(3);
  const auto Sk = k.size(1);
  const SegIds seg = seg_ids(q_seg, kv_seg, q, k);
  TORCH_CHECK(dout.size(0) == B && dout.size(1) == Sq && dout.size(2) == N &&
                  dout.size(3) == D,
              "dout/q shape mismatch");
  TORCH_CHECK(dout.scalar_type() == q.scalar_type(), "dout/q dtype mismatch");
  TORCH_CHECK(delta.scalar_type() == at::kFloat && lse.scalar_type() == at::kFloat,
              "delta/lse must be fp32");
  TORCH_CHECK(delta.dim() == 3 && lse.dim() == 3, "delta/lse must be [B,N,S]");
  TORCH_CHECK(delta.stride(2) == 1 && lse.stride(2) == 1,
              "delta/lse seq dim must be contiguous");
  TORCH_CHECK(delta.size(2) == Sq && lse.size(2) == Sq,
              "delta/lse seqlen mismatch");
  check_grad_out(dq, q, "dq");
  check_grad_out(dk, k, "dk");
  check_grad_out(dv, v, "dv");
  int64_t ds[2] = {delta.stride(0), delta.stride(1)};
  int64_t ls[2] = {lse.stride(0), lse.stride(1)};
  auto stream = at::hip::getCurrentHIPStream().stream();
  if (band_given(band_lo, band_hi, seg)) {
    BA_CALL(bahip_attn_bwd_band(
        dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
        delta.data_ptr<float>(), lse.data_ptr<float>(), dq.data_ptr<float>(),
        dk.data_ptr<float>(), dv.data_ptr<float>(), B, Sq, Sk, N, k.size(2), D,
        Strides3(dout), Strides3(q), Strides3(k), Strides3(v), ds, ls,
        Strides3(dq), Strides3(dk), Strides3(dv), (float)softmax_scale,
        causal ? 1 : 0, deterministic ? 1 : 0, dtype_code(q), *band_lo,
        *band_hi, stream));
    return;
  }
  BA_CALL(bahip_attn_bwd_seg(
      dout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
      delta.data_ptr<float>(), lse.data_ptr<float>(), dq.data_ptr<float>(),
      dk.data_ptr<float>(), dv.data_ptr<float>(), B, Sq, Sk, N, k.size(2), D,
      Strides3(dout), Strides3(q), Strides3(k), Strides3(v), ds, ls,
      Strides3(dq), Strides3(dk), Strides3(dv), (float)softmax_scale,
      causal ? 1 : 0, deterministic ? 1 : 0, dtype_code(q), seg.q, seg.kv,
      seg.q_sb, seg.kv_sb, seg.ws_ptr(), seg.ws_bytes(), stream));
}

std::vector<at::Tensor> attn_bwd(const at::Tensor& dout, const at::Tensor& q,
                                 const at::Tensor& k, const at::Tensor& v,
                                 const at::Tensor& delta,
                                 const at::Tensor& lse, double softmax_scale,
                                 bool causal, bool deterministic,
                                 const c10::optional<at::Tensor>& q_seg,
                                 const c10::optional<at::Tensor>& kv_seg,
                                 const c10::optional<int64_t>& band_lo,
                                 const c10::optional<int64_t>& band_hi) {
  const auto B = q.size(0), Sq = q.size(1), N = q.size(2), D = q.size(3);
  const auto Sk = k.size(1);
  // zero-filled: the kernels accumulate, so this equals fresh outputs
  auto dq = at::zeros({B, Sq, N, D}, q.options().dtype(at::kFloat));
  // dk/dv take k/v's head count (Nk <= N with grouped-query heads)
  const auto Nk = k.size(2);
  auto dk = at::zeros({B, Sk, Nk, D}, q.options().dtype(at::kFloat));
  auto dv = at::zeros({B, Sk, Nk, D}, q.options().dtype(at::kFloat));
  attn_bwd_accum(dout, q, k, v, delta, lse, softmax_scale, causal,
                 deterministic, dq, dk, dv, q_seg, kv_seg, band_lo, band_hi);
  return {dq, dk, dv};
}

// ---- hipModule side-load of the .s-built forward (round-3 on-ramp) ---
// attn_fwd_asm_load(path, symbol): load the hsaco once per process and
// bind the accum-form kernel; attn_fwd_accum_asm(...): same contract as
// attn_fwd_accum, dispatched through the module by
// bahip_attn_fwd_accum_fn (which packs the kernargs and derives the grid).
namespace {
hipModule_t g_asm_mod = nullptr;
std::string g_asm_path;
hipFunction_t g_asm_fn[2] = {nullptr, nullptr};  // [0]=f16, [1]=bf16

void attn_fwd_asm_load(const std::string& path, const std::string& sym_f16,
                       const std::string& sym_bf16) {
  if (g_asm_mod == nullptr || g_asm_path != path) {
    // earlier modules stay loaded (cheap); only the bound functions matter
    TORCH_CHECK(hipModuleLoad(&g_asm_mod, path.c_str()) == hipSuccess,
                "hipModuleLoad failed for ", path);
    g_asm_path = path;
  }
  TORCH_CHECK(hipModuleGetFunction(&g_asm_fn[0], g_asm_mod,
                                   sym_f16.c_str()) == hipSuccess,
              "symbol not found: ", sym_f16);
  TORCH_CHECK(hipModuleGetFunction(&g_asm_fn[1], g_asm_mod,
                                   sym_bf16.c_str()) == hipSuccess,
              "symbol not found: ", sym_bf16);
}

void attn_fwd_accum_asm(const at::Tensor& q, const at::Tensor& k,
                        const at::Tensor& v, double softmax_scale,
                        bool causal, at::Tensor& acc, at::Tensor& m,
                        at::Tensor& l, bool carry_in) {
  const int dt = dtype_code(q);
  TORCH_CHECK(g_asm_fn[dt] != nullptr, "asm forward not loaded");
  TORCH_CHECK(q.size(3) == 128, "asm forward: D=128 variants only");
  fwd_accum_call(g_asm_fn[dt], q, k, v, softmax_scale, causal, acc, m, l,
                 carry_in);
}
}  // namespace

at::Tensor mfma_probe(const at::Tensor& a, const at::Tensor& b) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.is_contiguous() && b.is_contiguous());
  TORCH_CHECK(a.sizes() == at::IntArrayRef({32, 16}) &&
              b.sizes() == at::IntArrayRef({16, 32}));
  auto d = at::zeros({32, 32}, a.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_mfma_probe(a.data_ptr(), b.data_ptr(), d.data_ptr<float>(),
                           dtype_code(a), stream));
  return d;
}

at::Tensor tr16_probe(int64_t mode) {
  auto out = at::zeros({256}, at::TensorOptions().dtype(at::kInt).device(at::kCUDA));
  auto stream = at::hip::getCurrentHIPStream().stream();
  BA_CALL(bahip_tr16_probe((int)mode, out.data_ptr<int>(), stream));
  return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("attn_fwd", &attn_fwd, "BurstAttention fwd tile (gfx950)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("q_seg") = py::none(),
        py::arg("kv_seg") = py::none(), py::arg("band_lo") = py::none(),
        py::arg("band_hi") = py::none());
  m.def("attn_fwd_accum", &attn_fwd_accum,
        "carry-in accumulator fwd tile (in-kernel LSE merge)", py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("acc"), py::arg("m"), py::arg("l"),
        py::arg("carry_in"), py::arg("q_seg") = py::none(),
        py::arg("kv_seg") = py::none(), py::arg("band_lo") = py::none(),
        py::arg("band_hi") = py::none());
  m.def("attn_fwd_state_init", &attn_fwd_state_init,
        "write the empty carry-in state (no key seen yet) into acc, m, l");
  m.def("attn_seg_prepass", &attn_seg_prepass,
        "segment-id pre-pass alone: the int32 workspace (tile summaries and "
        "block ranges of both side pairs)");
  m.def("attn_seg_workspace_bytes", &bahip_attn_seg_workspace_bytes,
        "bytes of the segment-id pre-pass workspace of a (B, Sq, Sk) call");
  m.def("attn_fwd_finalize", &attn_fwd_finalize,
        "o = acc/l (cast), lse from state");
  m.def("attn_vt_image", &attn_vt_image,
        "V^T image [B,Nk,ceil(Sk/64),D,64] the forward's pre-pass writes",
        py::arg("v"), py::arg("out") = py::none());
  m.def("attn_fwd_workspace_bytes", &bahip_attn_fwd_workspace_bytes,
        "V^T image bytes a forward of (B, Sq, Sk, N, Nk, D) allocates under "
        "the current knobs; 0 = in-kernel transpose");
  m.def("attn_bwd_preprocess", &attn_bwd_preprocess, "delta = rowsum(o*do)",
        py::arg("o"), py::arg("dout"), py::arg("out") = py::none());
  m.def("attn_bwd", &attn_bwd, "BurstAttention bwd tile (gfx950)",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("delta"), py::arg("lse"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("deterministic"),
        py::arg("q_seg") = py::none(), py::arg("kv_seg") = py::none(),
        py::arg("band_lo") = py::none(), py::arg("band_hi") = py::none());
  m.def("attn_bwd_accum", &attn_bwd_accum,
        "bwd tile accumulating into fp32 dq/dk/dv views", py::arg("dout"),
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("delta"),
        py::arg("lse"), py::arg("softmax_scale"), py::arg("causal"),
        py::arg("deterministic"), py::arg("dq"), py::arg("dk"), py::arg("dv"),
        py::arg("q_seg") = py::none(), py::arg("kv_seg") = py::none(),
        py::arg("band_lo") = py::none(), py::arg("band_hi") = py::none());
  m.def("mfma_probe", &mfma_probe, "32x32x16 MFMA layout probe");
  m.def("tr16_probe", &tr16_probe, "ds_read_tr16_b64 semantics probe");
  m.def("attn_fwd_asm_load", &attn_fwd_asm_load,
        "load the .s-built forward hsaco (round-3 on-ramp)");
  m.def("attn_fwd_accum_asm", &attn_fwd_accum_asm,
        "carry-in fwd via the hipModule-loaded .s kernel");
}

/* C-ABI of the MI355X-native BurstAttention tile kernels (gfx950).
 *
 * These entry points replace, one for one, the flash-attn CUDA extension
 * calls the reference makes on its default path:
 *   bahip_attn_fwd            <- _flash_attn_forward(q,k,v,...) -> (o, lse)
 *                                as called at reference
 *                                burst_attn/burst_utils.py:150-160
 *   bahip_attn_bwd_preprocess <- flash bwd delta precompute
 *                                (sum(o*do), cf. reference lao.py:247-269 and
 *                                burst_attn_interface.py:272-278)
 *   bahip_attn_bwd            <- _flash_attn_backward(do,q,k,v,o,lse,dq,dk,dv,
 *                                ..., softmax_d) as called at
 *                                burst_attn/burst_utils.py:211-248
 *
 * Conventions:
 *   - q/k/v/do: fp16 or bf16, logical layout [B, S, N, D]; strides are in
 *     ELEMENTS as {batch, seq, head}; the innermost head_dim D is assumed
 *     contiguous.  Arbitrary seq slices (zigzag halves, striped shifts) are
 *     expressed through the strides + base pointer.
 *   - o (forward out) is fp32 [B, Sq, N, D] contiguous; lse fp32 [B, N, Sq]
 *     contiguous (flash-attn layout, burst_utils.py:150-163).
 *   - lse/delta inputs to the backward may be seq-sliced: strides are
 *     {batch, head} in elements, seq stride is 1.
 *   - dq/dk/dv outputs are fp32 ACCUMULATORS, strided {batch, seq, head}
 *     (D contiguous): every call ADDS its tile contribution in place, so
 *     the ring layer accumulates rounds without elementwise-add passes.
 *     Pass zero-filled buffers for plain (non-accumulating) semantics.
 *   - deterministic is accepted for call compatibility and does not
 *     select a plan: the default plan ("split8": two-pass dq + split
 *     dV/dK, atomic-free) and BA_BWD_FUSED=1 are bitwise run-to-run
 *     identical by construction.  Only BA_BWD_FUSED=2, the flash-attn
 *     style fused dK+dQ experiment with atomic fp32 dq, is not.
 *   - causal implies Sq == Sk (equal-length tiles; the ring's zigzag /
 *     striped bookkeeping reduces every other case to non-causal tiles).
 *   - grouped-query heads (GQA/MQA): the *_gqa entry points take the KV
 *     head count Nk after N.  q/do/dq are [B, S, N, D]; k/v and dk/dv are
 *     [B, S, Nk, D] with N % Nk == 0 and G = N / Nk.  Query head h attends
 *     KV head h / G (the flash-attn convention).  dk/dv receive the sum
 *     over the G query heads of each group, accumulated inside one kernel
 *     in a fixed order (bitwise deterministic).  lse, delta and the
 *     carry-in state (acc, m, l) stay per query head.  The symbols without
 *     the suffix are the Nk = N case.  Nk < 1 or N % Nk != 0 returns
 *     BAHIP_ERR_UNSUPPORTED.  The BA_BWD_FUSED=1/2 and BA_BWD_DK_FLIP=1
 *     experiment plans are equal-heads only and return
 *     BAHIP_ERR_UNSUPPORTED when Nk != N.
 *   - segment ids (packed sequences): the *_seg entry points take
 *     q_seg int32 [B, Sq] and kv_seg int32 [B, Sk] (seq stride 1, a batch
 *     stride each in elements; a window of a longer row is a base pointer).
 *     Pair (q row i, kv row j) is visible iff q_seg[i] == kv_seg[j] and, with
 *     causal, the causal rule holds as well.  No id value is special: ids
 *     may be negative, sparse and unsorted.  Both pointers null is exactly
 *     the entry point without ids; one of the two null returns
 *     BAHIP_ERR_SEGMENT_IDS.  A pre-pass on `stream` writes, into
 *     seg_workspace (bahip_attn_seg_workspace_bytes(B, Sq, Sk) bytes, one
 *     size for forward and backward, reusable once the call is enqueued),
 *     the (min, max) id of every 64-row tile and per 256-row block the range
 *     of tiles whose (min, max) overlaps the block's; workgroups visit only
 *     that range and a wave skips a tile whose (min, max) misses its rows'.
 *     With non-decreasing ids on both sides a tile that shares no id with a
 *     block is neither loaded nor computed; for arbitrary ids the test is
 *     conservative and the results are still exact.  A q row that sees no
 *     key (possible in direct rectangular calls only; in the ring every row
 *     sees itself): the stateless forward gives o = 0, lse = -inf; a
 *     carry_in = 0 accumulate call leaves acc = 0, l = 0 and an m that later
 *     rounds merge correctly; a carry_in = 1 call leaves the row's state
 *     untouched; bahip_attn_fwd_finalize gives o = 0, lse = -inf for an
 *     l == 0 row; the backward adds exactly zero from and to such rows.
 *     Ids are supported by the default forward variant and the default
 *     backward plan only: with ids, a BA_FWD_* selection of another variant,
 *     BA_BWD_FUSED=1/2, BA_BWD_DK_FLIP=1 or BA_DQ_PIPE=1 returns
 *     BAHIP_ERR_UNSUPPORTED naming the knob, and nothing is launched.  The
 *     forward with ids transposes V in the kernel whatever BA_FWD_VT says
 *     (its V^T workspace argument is ignored) and never uses hip_function.
 *   - band (sliding windows): the *_band entry points take band_lo and
 *     band_hi.  Pair (q row i, kv row j) of the tensors passed is visible iff
 *     band_lo <= i - j <= band_hi; Sq != Sk is allowed, band_lo may be
 *     negative and either bound may be huge (they are clamped to +-2^30).
 *     With causal the band is cut at the diagonal, band_lo = max(band_lo, 0),
 *     and Sq == Sk is still demanded.  band_lo > band_hi returns
 *     BAHIP_ERR_BAND and launches nothing.  There is no pre-pass and no
 *     workspace: a workgroup computes the range of 64-row tiles that can hold
 *     a visible pair from its block index, the band and the two lengths, and
 *     a wave skips a tile that misses the band of its 32 rows.  A row that
 *     sees no key behaves exactly as with segment ids (o = 0, lse = -inf; an
 *     untouched carry-in state; exactly zero gradients).  A band is supported
 *     where segment ids are: another BA_FWD_* variant, BA_BWD_FUSED=1/2,
 *     BA_BWD_DK_FLIP=1 or BA_DQ_PIPE=1 returns BAHIP_ERR_UNSUPPORTED naming
 *     the knob, V is transposed in the kernel, and a module kernel
 *     (hip_function) is never used.  A band together with segment ids has no
 *     entry point.
 *   - stream is a hipStream_t.
 * Returns 0 on success; nonzero = error.  Every nonzero return sets the
 * calling thread's bahip_last_error() message and every success clears it.
 * Codes: the BAHIP_ERR_* values below; any other nonzero value is the
 * hipError_t of a failed kernel launch.
 */
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAHIP_F16 0
#define BAHIP_BF16 1

#define BAHIP_ERR_CAUSAL_SHAPE 1001   /* causal with Sq != Sk */
#define BAHIP_ERR_UNSUPPORTED 1002    /* head_dim not 64/128, dtype, or
                                         an invalid (N, Nk) head pair */
#define BAHIP_ERR_DTYPE_MISMATCH 1003 /* o / dout dtypes differ */
#define BAHIP_ERR_BAD_KNOB 1004       /* a BA_FWD_* knob, BA_BWD_FUSED,
                                         BA_BWD_DK_FLIP, BA_DQ_PIPE or
                                         BA_DKQ_DBG outside its set */
#define BAHIP_ERR_WORKSPACE 1005      /* V^T image workspace null or too
                                         small; nothing is launched */

#define BAHIP_ERR_SEGMENT_IDS 1006    /* one of q_seg / kv_seg is null */

#define BAHIP_ERR_BAND 1007           /* band_lo > band_hi */

const char* bahip_last_error(void);

int bahip_attn_fwd(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* stream);

/* bahip_attn_fwd with Nk KV heads (see "grouped-query heads" above) */
int bahip_attn_fwd_gqa(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* stream);

/* carry-in accumulator forward (in-kernel LSE merge; replaces the
 * per-round cuda_scale_out_lse_helper pass, burst_utils.py:20-33).
 * State: acc fp32 [B,S,N,D] (unnormalised O), m fp32 [B,N,S] (running max,
 * exp2 domain), l fp32 [B,N,S] (running sum); acc strided {b,s,h}, m/l
 * strided {b,h} with contiguous seq.  carry_in=0 initialises the state. */
int bahip_attn_fwd_accum(
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream);

/* bahip_attn_fwd_accum through a hipModule-loaded kernel: hip_function is
 * a hipFunction_t for a code object of the production accum variant
 * (D = 128, default BA_FWD_* knobs) for this dtype.  Same arguments and
 * checks; the knobs are not consulted.  A null hip_function is
 * bahip_attn_fwd_accum. */
int bahip_attn_fwd_accum_fn(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream);

/* bahip_attn_fwd_accum / bahip_attn_fwd_accum_fn with Nk KV heads:
 * hip_function null launches the in-binary variant the BA_FWD_* knobs
 * select, non-null the given module kernel. */
int bahip_attn_fwd_accum_gqa(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream);

/* ---- V^T image (burst_attn_amd/csrc/vt_image.h) -----------------------
 * The forward stages V into LDS transposed.  Every workgroup that visits a
 * kv tile repeats that transpose, ceil(Sq/256) * G times per tile; with a
 * workspace the forward instead runs a pre-pass that writes the transposed
 * tiles once ([B][Nk][ceil(Sk/64)][D][64] elements, pad columns zero) and
 * then copies them.  Results are bitwise those of the plain entry points.
 *
 * bahip_attn_vt_image_bytes: byte size of the image of a [B, Sk, Nk, D] V.
 * bahip_attn_fwd_workspace_bytes: what a forward call with these shapes
 *   wants as workspace under the current knobs: the image size where the
 *   image form would run, else 0 (BA_FWD_VT=0, an experiment variant, or
 *   BA_FWD_VT unset and ceil(Sq/256) * G below the measured threshold).
 * bahip_attn_fwd_gqa_ws / bahip_attn_fwd_accum_gqa_ws: the *_gqa forwards
 *   with a workspace.  A null workspace is the plain entry point.  With one,
 *   a call that the knobs route to the image form launches the pre-pass and
 *   then the forward on `stream`; the image is rebuilt on every call, and the
 *   workspace may be reused or freed (stream-ordered) once the call is
 *   enqueued.  A call routed to the in-kernel transpose ignores it.  A
 *   workspace smaller than bahip_attn_vt_image_bytes returns
 *   BAHIP_ERR_WORKSPACE and launches nothing.  A module kernel
 *   (hip_function non-null) always transposes in the kernel.
 * bahip_attn_vt_image: the pre-pass alone; v strided {batch, seq, head}.
 * BA_FWD_VT: 1 forces the image form wherever the default variant runs and
 *   a workspace is given, 0 forces the in-kernel transpose, unset is the auto
 *   rule; any other value returns BAHIP_ERR_BAD_KNOB. */
int64_t bahip_attn_vt_image_bytes(int64_t B, int64_t Nk, int64_t Sk,
                                  int64_t D);
int64_t bahip_attn_fwd_workspace_bytes(int64_t B, int64_t Sq, int64_t Sk,
                                       int64_t N, int64_t Nk, int64_t D);
int bahip_attn_vt_image(
    const void* v, void* image, int64_t image_bytes,
    int64_t B, int64_t Sk, int64_t Nk, int64_t D,
    const int64_t v_strides[3], int dtype, void* stream);
int bahip_attn_fwd_gqa_ws(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* workspace, int64_t workspace_bytes, void* stream);
int bahip_attn_fwd_accum_gqa_ws(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    void* workspace, int64_t workspace_bytes, void* stream);

/* o = acc / l cast to dtype; lse = ln(l) + m*ln2; contiguous full chunk */
int bahip_attn_fwd_finalize(
    const float* acc, const float* m, const float* l, void* o, float* lse,
    int64_t B, int64_t S, int64_t N, int64_t D, int dtype, void* stream);

int bahip_attn_bwd_preprocess(
    const void* o, const void* dout, float* delta,
    int64_t B, int64_t S, int64_t N, int64_t D,
    const int64_t o_strides[3], const int64_t do_strides[3],
    int o_dtype, int do_dtype, void* stream);

int bahip_attn_bwd(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse,
    float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t D,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3],
    float softmax_scale, int causal, int deterministic, int dtype,
    void* stream);

/* bahip_attn_bwd with Nk KV heads: dk/dv are [B, Sk, Nk, D] */
int bahip_attn_bwd_gqa(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse,
    float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3],
    float softmax_scale, int causal, int deterministic, int dtype,
    void* stream);

/* ---- segment ids (see "segment ids" above) -----------------------------
 * bahip_attn_fwd_gqa_ws, bahip_attn_fwd_accum_gqa_ws and bahip_attn_bwd_gqa
 * with per-token ids and the pre-pass workspace.  The segment workspace is
 * also named BAHIP_ERR_WORKSPACE when null or too small. */
int64_t bahip_attn_seg_workspace_bytes(int64_t B, int64_t Sq, int64_t Sk);
/* The pre-pass alone, both side pairs (what bahip_attn_bwd_seg runs; the
 * forwards run the q-owning pair only).  The workspace then holds, as
 * 32-bit words in this order: flags [2][B] (kv, q: the side's ids decrease
 * somewhere), kv tile (min, max) [B][ceil(Sk/64)][2], q block ranges
 * [B][ceil(Sq/256)][2] over kv tiles, q tile (min, max) [B][ceil(Sq/64)][2],
 * kv block ranges [B][ceil(Sk/256)][2] over q tiles. */
int bahip_attn_seg_prepass(
    const int32_t* q_seg, const int32_t* kv_seg,
    int64_t q_seg_stride, int64_t kv_seg_stride,
    int64_t B, int64_t Sq, int64_t Sk,
    void* seg_workspace, int64_t seg_workspace_bytes, void* stream);
int bahip_attn_fwd_seg(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* workspace, int64_t workspace_bytes,
    const int32_t* q_seg, const int32_t* kv_seg,
    int64_t q_seg_stride, int64_t kv_seg_stride,
    void* seg_workspace, int64_t seg_workspace_bytes, void* stream);
int bahip_attn_fwd_accum_seg(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    void* workspace, int64_t workspace_bytes,
    const int32_t* q_seg, const int32_t* kv_seg,
    int64_t q_seg_stride, int64_t kv_seg_stride,
    void* seg_workspace, int64_t seg_workspace_bytes, void* stream);
int bahip_attn_bwd_seg(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse,
    float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3],
    float softmax_scale, int causal, int deterministic, int dtype,
    const int32_t* q_seg, const int32_t* kv_seg,
    int64_t q_seg_stride, int64_t kv_seg_stride,
    void* seg_workspace, int64_t seg_workspace_bytes, void* stream);

/* ---- band (see "band" above) -------------------------------------------
 * bahip_attn_fwd_gqa, bahip_attn_fwd_accum_gqa and bahip_attn_bwd_gqa with a
 * band on the row indices of the tensors passed.  hip_function is accepted
 * for the signature's sake and ignored. */
int bahip_attn_fwd_band(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    int64_t band_lo, int64_t band_hi, void* stream);
int bahip_attn_fwd_accum_band(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    int64_t band_lo, int64_t band_hi, void* stream);
int bahip_attn_bwd_band(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse,
    float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3],
    float softmax_scale, int causal, int deterministic, int dtype,
    int64_t band_lo, int64_t band_hi, void* stream);

/* The empty state, "no key seen yet", over [B, S] rows of a carry-in state
 * (acc strided {b,s,h}, m/l strided {b,h}, as in bahip_attn_fwd_accum):
 * acc = 0, l = 0 and the m a carry_in = 0 call starts from.
 * bahip_attn_fwd_finalize of it gives o = 0, lse = -inf, and a later
 * carry_in = 1 call merges into it exactly as a carry_in = 0 call would have
 * initialised it. */
int bahip_attn_fwd_state_init(
    float* acc, float* m, float* l,
    int64_t B, int64_t S, int64_t N, int64_t D,
    const int64_t acc_strides[3], const int64_t ml_strides[2], void* stream);

#ifdef __cplusplus
}
#endif

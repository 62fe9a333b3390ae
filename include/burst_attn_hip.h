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
 *   - head_dim: D = 64 and 128 run the 8-wave kernels (256 rows per
 *     workgroup).  D = 256 runs a kernel set of its own, 4 waves per
 *     workgroup at one wave per SIMD, 128 rows per workgroup (forward and dq:
 *     grid ceil(Sq/128) x N x B; dK/dV: ceil(Sk/128) x Nk x B), through the
 *     same entry points: bahip_attn_fwd[_gqa][_ws], bahip_attn_fwd_accum[_gqa]
 *     [_ws], bahip_attn_fwd_finalize, bahip_attn_fwd_state_init,
 *     bahip_attn_bwd_preprocess and bahip_attn_bwd[_gqa], fp16 and bf16,
 *     causal and rectangular tiles, strided slices, GQA, the same state
 *     contract and the same bitwise-deterministic backward.  At D = 256 the
 *     forward transposes V in the kernel: a V^T workspace argument is
 *     ignored, bahip_attn_fwd_workspace_bytes returns 0 and BA_FWD_VT is not
 *     consulted.  Not available at D = 256, each returning
 *     BAHIP_ERR_UNSUPPORTED with a message that names what was asked, nothing
 *     launched: the *_seg entry points with ids and the *_band entry points;
 *     a non-null hip_function; a BA_FWD_* selection other than the default
 *     variant; BA_BWD_FUSED=1/2, BA_BWD_DK_FLIP=1, BA_DQ_PIPE=1.  A knob value
 *     outside its set is BAHIP_ERR_BAD_KNOB as everywhere.  Any other D
 *     (96 included) returns BAHIP_ERR_UNSUPPORTED.
 *   - softcap (logit soft-capping, the flash-attn `softcap` argument): the
 *     *_softcap entry points take a float softcap before stream.  With
 *     softcap > 0 pair (i, j) gets the score
 *     softcap * tanh(q_i.k_j * softmax_scale / softcap) in place of
 *     q_i.k_j * softmax_scale; the causal / rectangular rule of the call then
 *     applies as without it.  lse is the natural-log sum-exp of the capped
 *     scores, o, dq, dk and dv are those of softmax over the capped scores
 *     times V; the state contract, finalize, state init and the preprocess
 *     are unchanged, and a ring caps every round with the same value.
 *     softcap == 0 is exactly the entry point without it (image form, module
 *     kernel and knobs included); softcap < 0 or non-finite returns
 *     BAHIP_ERR_SOFTCAP and launches nothing.  Supported at D = 64, 128 and
 *     256 (each head_dim's own kernel set in a soft-capped form), fp16 and
 *     bf16, GQA, strided slices, and as bitwise deterministic in the backward
 *     as the plain kernels.  A cap is supported by the default forward
 *     variant and the default backward plan only: another BA_FWD_* selection,
 *     BA_BWD_FUSED=1/2, BA_BWD_DK_FLIP=1 or BA_DQ_PIPE=1 returns
 *     BAHIP_ERR_UNSUPPORTED naming the knob and softcap, nothing launched.
 *     The forward with a cap transposes V in the kernel whatever BA_FWD_VT
 *     says (its V^T workspace argument is ignored) and never uses
 *     hip_function.  A cap together with segment ids or a band has no entry
 *     point.
 *   - block masks (block-sparse attention): the *_blk entry points take,
 *     before stream, a byte mask [Bm][Hm][ceil(Sq/BS)][ceil(Sk/BS)] with its
 *     four element strides, its two leading extents, log2(BS) and a workspace
 *     of bahip_attn_blk_workspace_bytes(Bm, Hm, Sq, Sk) bytes.  Pair (i, j) is
 *     visible iff mask[b or 0][KV head of the q head, or 0][i / BS][j / BS] is
 *     nonzero, on top of causal (which still demands Sq == Sk).  A pre-pass
 *     on `stream` turns the mask into one list of 64-row tiles per 256-row
 *     block of the side a kernel owns, and the kernels' tile loops run over
 *     those lists: work follows the number of set blocks.  A q row whose
 *     blocks are all clear gets o = 0, lse = -inf (stateless), an untouched
 *     state (carry_in = 1) or an empty one (carry_in = 0), and adds nothing to
 *     any gradient; a key nobody sees gets nothing added to dk / dv.  A null
 *     mask, BS < 64 or not a power of two, Bm not in {1, B} or Hm not in
 *     {1, Nk} returns BAHIP_ERR_BLOCK_MASK; a null or too small workspace
 *     BAHIP_ERR_WORKSPACE; D = 256, another BA_FWD_* selection,
 *     BA_BWD_FUSED=1/2, BA_BWD_DK_FLIP=1 or BA_DQ_PIPE=1
 *     BAHIP_ERR_UNSUPPORTED naming what was asked.  Nothing is launched in
 *     any of these cases.  D = 64 / 128, fp16 and bf16, GQA, strided slices;
 *     the backward is as bitwise deterministic as the plain kernels.  The
 *     forward transposes V in the kernel whatever BA_FWD_VT says and never
 *     uses hip_function.  A block mask together with segment ids, a band or a
 *     cap has no entry point.
 *   - unequal widths (multi-head latent attention heads): the *_dv entry
 *     points take the v width Dv after D.  q, k, dq, dk are [.., D]; v, o,
 *     dO, the carry-in accumulator and dv are [.., Dv]; lse, delta, m and l
 *     are unchanged.  (D, Dv) = (192, 128) runs a kernel set of its own, 4
 *     waves per workgroup at one wave per SIMD, 128 rows per workgroup, fp16
 *     and bf16, causal and rectangular tiles, strided slices, GQA, the same
 *     state contract (bahip_attn_fwd_state_init, bahip_attn_fwd_finalize and
 *     bahip_attn_bwd_preprocess are called with D = 128, the width of what
 *     they touch) and the same bitwise-deterministic backward.  D == Dv is
 *     exactly the *_gqa entry point.  Any other pair returns
 *     BAHIP_ERR_UNSUPPORTED with a message naming both widths.  At (192, 128)
 *     a BA_FWD_* selection other than the default variant, BA_BWD_FUSED=1/2,
 *     BA_BWD_DK_FLIP=1, BA_DQ_PIPE=1 and a non-null hip_function return
 *     BAHIP_ERR_UNSUPPORTED naming what was asked; V is transposed in the
 *     kernel and BA_FWD_VT is not consulted; there is no segment-id, band,
 *     softcap or block-mask form.  Nothing is launched by a refused call.
 *   - FP8 (OCP e4m3, the gfx950 native 8-bit format): the *_f8 entry points
 *     are a forward of their own for q, k, v of dtype BAHIP_F8E4M3 at
 *     D = 128 (equal widths), causal and rectangular tiles, strided slices
 *     (strides in elements = bytes, seq and head strides multiples of 16),
 *     GQA, stateless and carry-in.  Real values are q8 * descale_q and so on
 *     (per-tensor descales, positive and finite); o / acc, m and l are fp32
 *     in real units with the state contract of every other forward, so
 *     bahip_attn_fwd_state_init and bahip_attn_fwd_finalize serve them at
 *     D = 128.  A pre-pass on `stream` writes the permuted V^T image of this
 *     call (attn_fp8.h) into `workspace`, at least
 *     bahip_attn_fwd_f8_workspace_bytes() bytes; a null or short one returns
 *     BAHIP_ERR_WORKSPACE.  A descale that is not positive and finite returns
 *     BAHIP_ERR_DESCALE, and so does one whose derived multipliers (the
 *     score scale, 16 / descale_v, descale_v / 16) are not.  The entry points
 *     carry one D: v rows are read D bytes wide, so a caller with a v of
 *     another width must refuse it itself.  A misaligned base or stride
 *     returns BAHIP_ERR_UNSUPPORTED naming the tensor and the stride.
 *     D != 128, another dtype code, a BA_FWD_* selection
 *     other than the default variant and a non-null hip_function return
 *     BAHIP_ERR_UNSUPPORTED naming what was asked.  Nothing is launched by a
 *     refused call.  There is no backward and no mask form.  Every other
 *     entry point keeps refusing BAHIP_F8E4M3 as an unknown dtype code.
 *   - Block-scaled FP8: the *_f8_scaled entry points are the *_f8 ones with
 *     the descales read from device memory, so that no value has to come back
 *     to the host: real values are q8 * descale_q[b][n][row], k8 *
 *     descale_k[b][n / G][k_tile0 + kv_row / 64] and v8 *
 *     descale_v[b][n / G][channel].  The tensors are fp32 with innermost
 *     stride 1 and {batch, head} element strides of their own, so slices of
 *     larger tensors are legal; descale_q and descale_v describe exactly the
 *     rows and channels passed, descale_k the 64-row tiles of k counted from
 *     k_tile0 (a k view therefore starts on a tile of the tensor that was
 *     quantised).  Every entry must be positive and finite: they live on the
 *     device and are not checked.  A null tensor or strides pointer, or a
 *     negative k_tile0, returns BAHIP_ERR_DESCALE; everything *_f8 refuses is
 *     refused alike, and nothing is launched by a refused call.  Outputs, the
 *     state contract and the workspace are those of *_f8.  The per-tensor
 *     entry points launch the kernels they launched before.
 *     bahip_attn_quantize_f8 produces such inputs from fp16 / bf16 at D = 128:
 *     x8 = round-to-nearest-even(x / scale) with scale = amax / 448 of the
 *     element's group (never below FLT_MIN, 1.0 for an all-zero group), in the
 *     three groupings above.  Misaligned bases or strides, another D, dtype
 *     or mode return BAHIP_ERR_UNSUPPORTED, a null tensor BAHIP_ERR_DESCALE, a
 *     short channel-mode workspace BAHIP_ERR_WORKSPACE.
 *   - ALiBi (the flash-attn `alibi_slopes` argument): the *_alibi entry
 *     points take, before stream, slopes (fp32, one per QUERY head, head
 *     stride 1), slopes_batch_stride (elements between batch rows, 0 = one row
 *     shared by the batch), pos_offset and pos_stride.  Pair (q row i, kv row
 *     j) of the tensors passed gets the score
 *     q_i.k_j * softmax_scale - slopes[b][h] * |pos_stride * (i - j) +
 *     pos_offset|; the causal / rectangular rule of the call then applies as
 *     without it.  The two integers place the tensors in a longer sequence: a
 *     contiguous pair of pieces has pos_stride = 1 and pos_offset = (global
 *     position of q row 0) - (that of kv row 0); rows dealt round-robin to W
 *     ranks have pos_stride = W.  lse is the natural-log sum-exp of the biased
 *     scores, o, dq, dk and dv are those of softmax over the biased scores
 *     times V, the slopes get no gradient; the state contract, finalize, state
 *     init and the preprocess are unchanged, so rounds with different offsets
 *     merge through (acc, m, l) as plain rounds do.  The bias is computed in
 *     registers from the accumulator position, two FMAs per score; nothing is
 *     read but one slope per workgroup (per group member in dK/dV).  Null
 *     slopes is exactly the *_gqa entry point.  pos_stride < 1, or
 *     |pos_offset| + pos_stride * max(Sq, Sk) above 2^30 (the distance is an
 *     int32), returns BAHIP_ERR_ALIBI.  D = 64 / 128, fp16 and bf16, GQA,
 *     strided slices; the backward is as bitwise deterministic as the plain
 *     kernels.  D = 256, a BA_FWD_* selection other than the default variant,
 *     BA_BWD_FUSED=1/2, BA_BWD_DK_FLIP=1, BA_DQ_PIPE=1 and a non-null
 *     hip_function return BAHIP_ERR_UNSUPPORTED naming what was asked.
 *     Nothing is launched by a refused call.  The forward transposes V in the
 *     kernel whatever BA_FWD_VT says.  Slopes together with segment ids, a
 *     band, a cap, a block mask, unequal widths or fp8 have no entry point.
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
#define BAHIP_F8E4M3 2 /* the *_f8 entry points only */

#define BAHIP_ERR_CAUSAL_SHAPE 1001   /* causal with Sq != Sk */
#define BAHIP_ERR_UNSUPPORTED 1002    /* head_dim not 64/128/256, dtype, a
                                         form D = 256 does not have, or
                                         an invalid (N, Nk) head pair */
#define BAHIP_ERR_DTYPE_MISMATCH 1003 /* o / dout dtypes differ */
#define BAHIP_ERR_BAD_KNOB 1004       /* a BA_FWD_* knob, BA_BWD_FUSED,
                                         BA_BWD_DK_FLIP, BA_DQ_PIPE or
                                         BA_DKQ_DBG outside its set */
#define BAHIP_ERR_WORKSPACE 1005      /* V^T image workspace null or too
                                         small; nothing is launched */

#define BAHIP_ERR_SEGMENT_IDS 1006    /* one of q_seg / kv_seg is null */

#define BAHIP_ERR_BAND 1007           /* band_lo > band_hi */

#define BAHIP_ERR_SOFTCAP 1008        /* softcap negative or not finite */

#define BAHIP_ERR_BLOCK_MASK 1009     /* block mask null, BS < 64 or not a
                                         power of two, Bm not in {1, B}, Hm
                                         not in {1, Nk} */

#define BAHIP_ERR_DESCALE 1010        /* an fp8 descale not positive or not
                                         finite, or a null descale tensor */

#define BAHIP_ERR_ALIBI 1011          /* pos_stride < 1, or a position
                                         distance beyond 2^30 */

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

/* ---- softcap (see "softcap" above) --------------------------------------
 * bahip_attn_fwd_gqa_ws, bahip_attn_fwd_accum_gqa_ws and bahip_attn_bwd_gqa
 * with logit soft-capping. */
int bahip_attn_fwd_softcap(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* workspace, int64_t workspace_bytes, float softcap, void* stream);
int bahip_attn_fwd_accum_softcap(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    void* workspace, int64_t workspace_bytes, float softcap, void* stream);
int bahip_attn_bwd_softcap(
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
    float softcap, void* stream);

/* ---- ALiBi (see "ALiBi" above) --------------------------------------------
 * bahip_attn_fwd_gqa, bahip_attn_fwd_accum_gqa and bahip_attn_bwd_gqa with
 * per-head linear position biases. */
int bahip_attn_fwd_alibi(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    const float* slopes, int64_t slopes_batch_stride, int64_t pos_offset,
    int64_t pos_stride, void* stream);
int bahip_attn_fwd_accum_alibi(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    const float* slopes, int64_t slopes_batch_stride, int64_t pos_offset,
    int64_t pos_stride, void* stream);
int bahip_attn_bwd_alibi(
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
    const float* slopes, int64_t slopes_batch_stride, int64_t pos_offset,
    int64_t pos_stride, void* stream);

/* ---- block masks (see "block masks" above) --------------------------------
 * bahip_attn_fwd_gqa, bahip_attn_fwd_accum_gqa and bahip_attn_bwd_gqa with a
 * block mask.  The workspace holds, in 32-bit words, with L = Bm * Hm,
 * nb(S) = ceil(S / 256) and nt(S) = ceil(S / 64):
 *   q_cnt [L][nb(Sq)], q_list [L][nb(Sq)][nt(Sk)]   (forward, dq)
 *   kv_cnt [L][nb(Sk)], kv_list [L][nb(Sk)][nt(Sq)] (dK, dV)
 * a list's first cnt entries being (tile index | wave mask << 24), ascending.
 * bahip_attn_blk_prepass writes both sides alone, for tests and measurements;
 * the forward writes the q side, the backward both. */
int64_t bahip_attn_blk_workspace_bytes(int64_t Bm, int64_t Hm, int64_t Sq,
                                       int64_t Sk);
int bahip_attn_blk_prepass(
    const uint8_t* block_mask, const int64_t mask_strides[4], int64_t Bm,
    int64_t Hm, int log2_block_size, int64_t Sq, int64_t Sk, int causal,
    void* blk_workspace, int64_t blk_workspace_bytes, void* stream);
int bahip_attn_fwd_blk(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    const uint8_t* block_mask, const int64_t mask_strides[4], int64_t Bm,
    int64_t Hm, int log2_block_size, void* blk_workspace,
    int64_t blk_workspace_bytes, void* stream);
int bahip_attn_fwd_accum_blk(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    const uint8_t* block_mask, const int64_t mask_strides[4], int64_t Bm,
    int64_t Hm, int log2_block_size, void* blk_workspace,
    int64_t blk_workspace_bytes, void* stream);
int bahip_attn_bwd_blk(
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
    const uint8_t* block_mask, const int64_t mask_strides[4], int64_t Bm,
    int64_t Hm, int log2_block_size, void* blk_workspace,
    int64_t blk_workspace_bytes, void* stream);

/* ---- unequal widths (see "unequal widths" above) -------------------------
 * bahip_attn_fwd_gqa, bahip_attn_fwd_accum_gqa and bahip_attn_bwd_gqa with the
 * v width Dv after D. */
int bahip_attn_fwd_dv(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    void* stream);
int bahip_attn_fwd_accum_dv(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in, void* stream);
int bahip_attn_bwd_dv(
    const void* dout, const void* q, const void* k, const void* v,
    const float* delta, const float* lse,
    float* dq, float* dk, float* dv,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    int64_t Dv,
    const int64_t do_strides[3], const int64_t q_strides[3],
    const int64_t k_strides[3], const int64_t v_strides[3],
    const int64_t delta_strides[2], const int64_t lse_strides[2],
    const int64_t dq_strides[3], const int64_t dk_strides[3],
    const int64_t dv_strides[3],
    float softmax_scale, int causal, int deterministic, int dtype,
    void* stream);

/* ---- FP8 e4m3 forward (see "FP8" above) -----------------------------------
 * The GQA argument lists with the three per-tensor descales and the V^T image
 * workspace.  BAHIP_F8_P_SCALE is the power of two the kernel multiplies P by
 * before it rounds P to e4m3 (attn_fp8.h: BA_FP8_PSCALE). */
#define BAHIP_F8_P_SCALE 16
int64_t bahip_attn_fwd_f8_workspace_bytes(int64_t B, int64_t Sk, int64_t Nk,
                                          int64_t D);
int bahip_attn_fwd_f8(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    float descale_q, float descale_k, float descale_v,
    void* workspace, int64_t workspace_bytes, void* stream);
int bahip_attn_fwd_accum_f8(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    float descale_q, float descale_k, float descale_v,
    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- block-scaled FP8 forward and its quantiser (see "Block-scaled FP8") ----
 * The *_f8 argument lists with the three floats replaced by three fp32 device
 * tensors (innermost stride 1), their {batch, head} element strides and
 * k_tile0, the descale_k index of the call's first 64-row kv tile:
 *   descale_q [B][N][Sq], descale_k [B][Nk][>= k_tile0 + ceil(Sk/64)],
 *   descale_v [B][Nk][128]. */
int bahip_attn_fwd_f8_scaled(
    const void* q, const void* k, const void* v,
    float* o, float* lse,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3],
    const int64_t k_strides[3],
    const int64_t v_strides[3],
    float softmax_scale, int causal, int dtype,
    const float* descale_q, const float* descale_k, const float* descale_v,
    const int64_t dq_strides[2], const int64_t dk_strides[2],
    const int64_t dv_strides[2], int64_t k_tile0,
    void* workspace, int64_t workspace_bytes, void* stream);
int bahip_attn_fwd_accum_f8_scaled(
    void* hip_function,
    const void* q, const void* k, const void* v,
    int64_t B, int64_t Sq, int64_t Sk, int64_t N, int64_t Nk, int64_t D,
    const int64_t q_strides[3], const int64_t k_strides[3],
    const int64_t v_strides[3], float softmax_scale, int causal, int dtype,
    float* acc, float* m, float* l, const int64_t acc_strides[3],
    const int64_t ml_strides[2], int carry_in,
    const float* descale_q, const float* descale_k, const float* descale_v,
    const int64_t dq_strides[2], const int64_t dk_strides[2],
    const int64_t dv_strides[2], int64_t k_tile0,
    void* workspace, int64_t workspace_bytes, void* stream);

/* x (fp16 / bf16 [B][S][H][128], element strides {b, s, h}) -> x8 (e4m3
 * bytes, byte strides {b, s, h}) and `scale`, contiguous fp32:
 *   BAHIP_F8_QUANT_ROW      [B][H][S]             one per row (q)
 *   BAHIP_F8_QUANT_TILE     [B][H][ceil(S/64)]    one per 64-row tile (k)
 *   BAHIP_F8_QUANT_CHANNEL  [B][H][128]           one per channel (v)
 * Only the channel mode needs a workspace. */
#define BAHIP_F8_QUANT_ROW 0
#define BAHIP_F8_QUANT_TILE 1
#define BAHIP_F8_QUANT_CHANNEL 2
int64_t bahip_attn_quantize_f8_workspace_bytes(int mode, int64_t B, int64_t S,
                                               int64_t H);
int bahip_attn_quantize_f8(
    const void* x, void* x8, float* scale,
    int64_t B, int64_t S, int64_t H, int64_t D,
    const int64_t x_strides[3], const int64_t x8_strides[3],
    int dtype, int mode,
    void* workspace, int64_t workspace_bytes, void* stream);

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

// Backward kernel-plan selection: BA_BWD_* / BA_DQ_PIPE / BA_DKQ_DBG knob
// values and the group size G -> the ordered list of kernels bahip_attn_bwd
// launches.  Host-only and free of HIP includes, so a plain C++17 compiler
// can build it (tests/test_bwd_plan_table_cpu.py does).  What each plan
// computes: the top of attn_bwd.hip; what was measured: DESIGN.md.
#pragma once

struct ba_bwd_knobs {
  int fused = 0;    // 0 = split8 (default), 1 = dkvf7, 2 = atomic6
  int dk_flip = 0;  // split8 only: flipped dK kernel
  int dq_pipe = 0;  // dq kernel with LDS-imaged dO + read-ahead
  int dkq_dbg = 0;  // atomic6 only: perf probes (results wrong for > 0)
};

// Each knob accepts 0..max, in ba_bwd_knobs field order.
constexpr struct {
  const char* env;
  int max;
} BA_BWD_KNOB_SPECS[4] = {
    {"BA_BWD_FUSED", 2}, {"BA_BWD_DK_FLIP", 1}, {"BA_DQ_PIPE", 1},
    {"BA_DKQ_DBG", 2}};

// Every kernel bahip_attn_bwd can launch; each names one instantiation family.
enum ba_bwd_step {
  BA_STEP_DQ,           // bwd_dq_kernel<DQP=0>
  BA_STEP_DQ_PIPE,      // bwd_dq_kernel<DQP=1>
  BA_STEP_DV,           // bwd_dkv_kernel<MODE=0> (GQA form when G > 1)
  BA_STEP_DK,           // bwd_dkv_kernel<MODE=1> (GQA form when G > 1)
  BA_STEP_DK_FLIPPED,   // bwd_dkq_kernel<FUSE_DQ=0>
  BA_STEP_DKDV_FUSED,   // bwd_dkq_kernel<0, 0, 32, FUSE_DV=1>
  BA_STEP_DKDQ_ATOMIC,  // bwd_dkq_kernel<FUSE_DQ=1, DBG=0>
  BA_STEP_DKDQ_DBG1,    // bwd_dkq_kernel<1, DBG=1>
  BA_STEP_DKDQ_DBG2,    // bwd_dkq_kernel<1, DBG=2>
};

// BAD_VALUE: `knob` holds a `value` outside its accepted set; NO_GQA: it
// is equal-heads only and G > 1.  OK: `steps` lists the launches in order.
enum ba_bwd_verdict { BA_BWD_OK, BA_BWD_BAD_VALUE, BA_BWD_NO_GQA };
struct ba_bwd_plan {
  ba_bwd_verdict verdict;
  const char* knob;
  int value;
  int n_steps;
  ba_bwd_step steps[3];
};

// Knobs a plan does not use are validated but otherwise ignored: DKQ_DBG
// outside atomic6, DQ_PIPE under atomic6 (it has no dq kernel), DK_FLIP
// outside split8.  The bwd_dkq_kernel family is equal-heads only.
constexpr ba_bwd_plan ba_bwd_select(const ba_bwd_knobs& k, int G) {
  const int vals[4] = {k.fused, k.dk_flip, k.dq_pipe, k.dkq_dbg};
  for (int i = 0; i < 4; ++i)
    if (vals[i] < 0 || vals[i] > BA_BWD_KNOB_SPECS[i].max)
      return {BA_BWD_BAD_VALUE, BA_BWD_KNOB_SPECS[i].env, vals[i], 0, {}};
  if (G > 1 && k.fused)
    return {BA_BWD_NO_GQA, BA_BWD_KNOB_SPECS[0].env, k.fused, 0, {}};
  if (G > 1 && k.dk_flip)
    return {BA_BWD_NO_GQA, BA_BWD_KNOB_SPECS[1].env, k.dk_flip, 0, {}};
  const ba_bwd_step dq = k.dq_pipe ? BA_STEP_DQ_PIPE : BA_STEP_DQ;
  if (k.fused == 1) return {BA_BWD_OK, nullptr, 0, 2, {dq, BA_STEP_DKDV_FUSED}};
  if (k.fused == 2)
    return {BA_BWD_OK, nullptr, 0, 2,
            {BA_STEP_DV, k.dkq_dbg == 1   ? BA_STEP_DKDQ_DBG1
                         : k.dkq_dbg == 2 ? BA_STEP_DKDQ_DBG2
                                          : BA_STEP_DKDQ_ATOMIC}};
  return {BA_BWD_OK, nullptr, 0, 3,
          {dq, BA_STEP_DV, k.dk_flip ? BA_STEP_DK_FLIPPED : BA_STEP_DK}};
}

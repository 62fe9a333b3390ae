#!/usr/bin/env python3
"""Benchmark sweep — reproduces the reference's measurement methodology
(benchmarks/benchmark.py: warmup + timed mean, FLOPs model :17-24, per-GPU
TFLOPS = FLOPs/time/1e12/world_size :204-209, jsonlines rows :286-298).

Single node:
  python benchmarks/sweep.py                      # 1 GPU
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 \
      benchmarks/sweep.py --configs ring          # 8-GPU ring rows

Grouped-query attention:
  python benchmarks/sweep.py --configs gqa --kv-heads 8
runs, at s=65536, the equal-heads row, the --kv-heads row (same FLOPs,
counted on the query heads; fewer K/V bytes) and the backward tile both
as the in-kernel group loop and as the G-launch comparator.  --kv-heads
also applies to the other burst configs.

Packed sequences (segment ids):
  python benchmarks/sweep.py --configs packed --doc-len 8192
runs, at --seq (65536), dense causal, the packed causal sequence of
--doc-len documents (repeat the option or give a comma list for mixed
lengths, cycled until the sequence is full), for one uniform length the
b = seq / doc-len batch of single documents (the same visible work), and
the segment pre-pass alone at 65536 and 1048576 tokens.  TFLOPS of the
packed rows count the visible pairs only.

Sliding windows:
  python benchmarks/sweep.py --window 4096 --window 16384
runs, at --seq (65536), dense causal and then causal with each --window
L[,R] (window_size=(L, R); R defaults to 0), and reports next to each time
its ratio to the dense causal row and the ideal ratio: the (256-row block,
64-row tile) pairs that hold a visible pair under the window, over those
under the causal triangle, counted with the arithmetic of
csrc/band_support.h.  TFLOPS of the window rows count the visible pairs only.

Row fields mirror the reference's results_torch.jsonl semantics.
"""

import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.distributed as dist


def flops_fwd(b, s, n, d, causal):
    f = 4.0 * b * s * s * n * d  # reference benchmark.py:17-24
    return f / 2 if causal else f


def timeit(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    t = torch.tensor([dt], dtype=torch.float64, device="cuda")
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def bench_burst(args, b, s_global, n, d, causal, striped, opt_bwd, steps, warmup,
                nk=None):
    from burst_attn_amd import burst_attn_func, burst_attn_func_striped

    world = dist.get_world_size()
    rank = dist.get_rank()
    s_local = s_global // world
    nk = n if nk is None else nk
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    g = torch.Generator().manual_seed(1000 + rank)
    mk = lambda h=n: torch.randn(b, s_local, h, d, generator=g).to(dtype).cuda()
    q, k, v, do = mk(), mk(nk), mk(nk), mk()
    func = burst_attn_func_striped if striped else burst_attn_func

    def fwd():
        with torch.no_grad():
            func(q, k, v, None, "cuda", causal, opt_bwd)

    def fwdbwd():
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))
        o = func(qg, kg, vg, None, "cuda", causal, opt_bwd)
        torch.autograd.grad(o, (qg, kg, vg), do)

    t_f = timeit(fwd, steps, warmup)
    t_fb = timeit(fwdbwd, steps, warmup)
    f = flops_fwd(b, s_global, n, d, causal)
    return {
        "method": "burst_striped" if striped else "burst",
        "b": b, "s": s_global, "n": n, "nk": nk, "d": d,
        "causal": causal, "opt_bwd": opt_bwd, "wsize": world,
        "dtype": args.dtype,
        "fwd_ms": round(t_f * 1e3, 2),
        "fwd_tflops_per_gpu": round(f / t_f / 1e12 / world, 2),
        "fwdbwd_ms": round(t_fb * 1e3, 2),
        "fwdbwd_tflops_per_gpu": round(3.5 * f / t_fb / 1e12 / world, 2),
    }


def packed_cu(s, doc_lens):
    """cu_seqlens of `doc_lens` cycled until s tokens are covered (the last
    document is cut at s)."""
    cu, i = [0], 0
    while cu[-1] < s:
        cu.append(min(s, cu[-1] + doc_lens[i % len(doc_lens)]))
        i += 1
    return cu


def bench_packed(args, s, n, nk, d, doc_lens, steps, warmup):
    """Causal forward and forward+backward of one packed sequence through
    burst_attn_func(segment_ids=...)."""
    from burst_attn_amd import burst_attn_func, segment_ids_from_cu_seqlens

    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    g = torch.Generator().manual_seed(1000)
    mk = lambda h=n: torch.randn(1, s, h, d, generator=g).to(dtype).cuda()
    q, k, v, do = mk(), mk(nk), mk(nk), mk()
    cu = packed_cu(s, doc_lens)
    ids = segment_ids_from_cu_seqlens(cu, s).unsqueeze(0).cuda()

    def fwd():
        with torch.no_grad():
            burst_attn_func(q, k, v, None, "cuda", True, segment_ids=ids)

    def fwdbwd():
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))
        o = burst_attn_func(qg, kg, vg, None, "cuda", True, segment_ids=ids)
        torch.autograd.grad(o, (qg, kg, vg), do)

    t_f = timeit(fwd, steps, warmup)
    t_fb = timeit(fwdbwd, steps, warmup)
    pairs = sum((b - a) * (b - a) for a, b in zip(cu[:-1], cu[1:])) / 2
    f = 4.0 * pairs * n * d
    return {
        "method": "burst_packed", "b": 1, "s": s, "n": n, "nk": nk, "d": d,
        "causal": True, "doc_lens": doc_lens, "docs": len(cu) - 1,
        "visible_frac": round(pairs / (s * s / 2), 4), "wsize": 1,
        "dtype": args.dtype,
        "fwd_ms": round(t_f * 1e3, 2),
        "fwd_tflops_per_gpu": round(f / t_f / 1e12, 2),
        "fwdbwd_ms": round(t_fb * 1e3, 2),
        "fwdbwd_tflops_per_gpu": round(3.5 * f / t_fb / 1e12, 2),
    }


def band_tile_pairs(lo, hi, s_own, s_str):
    """csrc/band_support.h's ba_band_tile_pairs, restated: the (256-row own
    block, 64-row streamed tile) pairs that hold a pair with
    lo <= own - streamed <= hi (tests/test_band_support_cpu.py pins this to
    the header)."""
    n = 0
    for r0 in range(0, s_own, 256):
        r1 = min(r0 + 255, s_own - 1)
        s0, s1 = max(r0 - hi, 0), min(r1 - lo, s_str - 1)
        if lo <= hi and s0 <= s1:
            n += s1 // 64 - s0 // 64 + 1
    return n


def bench_window(args, s, n, nk, d, window, dense, steps, warmup):
    """Causal forward and forward+backward under window_size=window, next to
    the dense causal row `dense` of the same run."""
    from burst_attn_amd import burst_attn_func

    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    g = torch.Generator().manual_seed(1000)
    mk = lambda h=n: torch.randn(1, s, h, d, generator=g).to(dtype).cuda()
    q, k, v, do = mk(), mk(nk), mk(nk), mk()

    def fwd():
        with torch.no_grad():
            burst_attn_func(q, k, v, None, "cuda", True, window_size=window)

    def fwdbwd():
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))
        o = burst_attn_func(qg, kg, vg, None, "cuda", True,
                            window_size=window)
        torch.autograd.grad(o, (qg, kg, vg), do)

    t_f = timeit(fwd, steps, warmup)
    t_fb = timeit(fwdbwd, steps, warmup)
    left = window[0]
    hi = s if left < 0 else left
    i = torch.arange(s, dtype=torch.float64)
    pairs = float((torch.minimum(i, torch.full_like(i, hi)) + 1).sum())
    f = 4.0 * pairs * n * d
    big = 1 << 30
    ideal = band_tile_pairs(0, hi, s, s) / band_tile_pairs(0, big, s, s)
    return {
        "method": "burst_window", "b": 1, "s": s, "n": n, "nk": nk, "d": d,
        "causal": True, "window": list(window), "wsize": 1,
        "visible_frac": round(pairs / (s * (s + 1) / 2), 4),
        "ideal_tile_ratio": round(ideal, 4),
        "dtype": args.dtype,
        "fwd_ms": round(t_f * 1e3, 2),
        "fwd_ratio_to_causal": round(t_f * 1e3 / dense["fwd_ms"], 4),
        "fwd_tflops_per_gpu": round(f / t_f / 1e12, 2),
        "fwdbwd_ms": round(t_fb * 1e3, 2),
        "fwdbwd_ratio_to_causal": round(t_fb * 1e3 / dense["fwdbwd_ms"], 4),
        "fwdbwd_tflops_per_gpu": round(3.5 * f / t_fb / 1e12, 2),
    }


def bench_seg_prepass(args, s, doc_len, steps, warmup):
    """The segment pre-pass alone (both side pairs, as the backward runs
    it; the forward runs half of it)."""
    from burst_attn_amd import segment_ids_from_cu_seqlens
    from burst_attn_amd._ext import load_extension

    ext = load_extension()
    ids = segment_ids_from_cu_seqlens(packed_cu(s, [doc_len]), s)
    ids = ids.unsqueeze(0).cuda()
    t = timeit(lambda: ext.attn_seg_prepass(ids, ids), steps, warmup)
    return {"method": "seg_prepass", "b": 1, "s": s, "doc_lens": [doc_len],
            "wsize": 1, "prepass_us": round(t * 1e6, 1)}


def bench_bwd_tile(args, b, s, n, nk, d, causal, g_launch, steps, warmup):
    """Backward tile alone (dq + dV + dK kernels, accumulating form).

    g_launch=False: one call with Nk-head k/v — the in-kernel group loop.
    g_launch=True: the comparator — the same tile as G = n // nk calls of
    the equal-heads path on strided head views (q/do/dq ``[:, :, g::G]``,
    delta/lse ``[:, g::G]``, the same dk/dv): K/V are re-loaded and dk/dv
    read-modify-written G times."""
    from burst_attn_amd._ext import load_extension

    ext = load_extension()
    G = n // nk
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    gen = torch.Generator().manual_seed(11)
    mk = lambda h: torch.randn(b, s, h, d, generator=gen).to(dtype).cuda()
    q, k, v, do = mk(n), mk(nk), mk(nk), mk(n)
    scale = 1.0 / math.sqrt(d)
    o, lse = ext.attn_fwd(q, k, v, scale, causal)
    delta = ext.attn_bwd_preprocess(o.to(dtype), do)
    del o
    dq = torch.zeros(b, s, n, d, dtype=torch.float32, device="cuda")
    dk = torch.zeros(b, s, nk, d, dtype=torch.float32, device="cuda")
    dv = torch.zeros_like(dk)

    def grouped():
        ext.attn_bwd_accum(do, q, k, v, delta, lse, scale, causal, True,
                           dq, dk, dv)

    def launches():
        for g in range(G):
            ext.attn_bwd_accum(do[:, :, g::G], q[:, :, g::G], k, v,
                               delta[:, g::G], lse[:, g::G], scale, causal,
                               True, dq[:, :, g::G], dk, dv)

    t = timeit(launches if g_launch else grouped, steps, warmup)
    f = 2.5 * flops_fwd(b, s, n, d, causal)  # bwd = 3.5x - 1x fwd
    return {
        "method": "bwd_tile_g_launch" if g_launch else "bwd_tile_group_loop",
        "b": b, "s": s, "n": n, "nk": nk, "d": d, "causal": causal,
        "wsize": 1, "dtype": args.dtype,
        "bwd_ms": round(t * 1e3, 2),
        "bwd_tflops_per_gpu": round(f / t / 1e12, 2),
    }


def bench_single_flash(args, b, s, n, d, causal, steps, warmup):
    """Single-GPU full-sequence tile — the reference README's
    'flash single GPU' comparator column, using our own fwd kernel."""
    from burst_attn_amd._ext import load_extension

    ext = load_extension()
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    g = torch.Generator().manual_seed(7)
    mk = lambda: torch.randn(b, s, n, d, generator=g).to(dtype).cuda()
    q, k, v = mk(), mk(), mk()
    scale = 1.0 / math.sqrt(d)
    fn = lambda: ext.attn_fwd(q, k, v, scale, causal)
    t_f = timeit(fn, steps, warmup)
    f = flops_fwd(b, s, n, d, causal)
    return {
        "method": "flash_single_gpu", "b": b, "s": s, "n": n, "d": d,
        "causal": causal, "wsize": 1, "dtype": args.dtype,
        "fwd_ms": round(t_f * 1e3, 2),
        "fwd_tflops_per_gpu": round(f / t_f / 1e12, 2),
    }


def bench_ring_naive(args, b, s_global, n, d, steps, warmup):
    """RingQK/RingAV comparator column (reference benchmarks/ring_attn.py;
    restated in benchmarks/ring_naive.py).  Materialises the full score
    slab — configs must fit O(S^2/W) per rank."""
    from benchmarks.ring_naive import ring_naive_attention, slab_bytes

    world = dist.get_world_size()
    rank = dist.get_rank()
    s_local = s_global // world
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    need = 4 * slab_bytes(b, n, s_local, s_global, dtype)  # slab+probs+grads
    free = torch.cuda.mem_get_info()[0]
    if need > free * 0.6:
        return None
    g = torch.Generator().manual_seed(2000 + rank)
    mk = lambda: torch.randn(b * n, s_local, d, generator=g).to(dtype).cuda()
    q, k, v, do = mk(), mk(), mk(), mk()
    scale = 1.0 / math.sqrt(d)

    def fwd():
        with torch.no_grad():
            ring_naive_attention(q, k, v, scale)

    def fwdbwd():
        qg, kg, vg = (t.detach().requires_grad_() for t in (q, k, v))
        o = ring_naive_attention(qg, kg, vg, scale)
        torch.autograd.grad(o, (qg, kg, vg), do)

    t_f = timeit(fwd, steps, warmup)
    t_fb = timeit(fwdbwd, steps, warmup)
    f = flops_fwd(b, s_global, n, d, False)
    return {
        "method": "ring_naive", "b": b, "s": s_global, "n": n, "d": d,
        "causal": False, "wsize": world, "dtype": args.dtype,
        "fwd_ms": round(t_f * 1e3, 2),
        "fwd_tflops_per_gpu": round(f / t_f / 1e12 / world, 2),
        "fwdbwd_ms": round(t_fb * 1e3, 2),
        "fwdbwd_tflops_per_gpu": round(3.5 * f / t_fb / 1e12 / world, 2),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs",
                   choices=["quick", "ring", "batch", "single", "naive", "gqa",
                            "packed"],
                   default="quick")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--dtype", choices=["fp16", "bf16"], default="fp16")
    p.add_argument("--out", default="results_mi355x.jsonl")
    p.add_argument("--heads", type=int, default=32)
    p.add_argument("--kv-heads", type=int, default=None,
                   help="K/V heads (default: equal to --heads)")
    p.add_argument("--seq", type=int, default=65536,
                   help="sequence length of the gqa and packed configs")
    p.add_argument("--doc-len", action="append", default=None,
                   help="packed config: document length(s); repeat or give "
                        "a comma list for mixed lengths (default 8192)")
    p.add_argument("--window", action="append", default=None,
                   metavar="L[,R]",
                   help="run dense causal at --seq and causal with "
                        "window_size=(L, R) (R defaults to 0); repeatable; "
                        "replaces --configs")
    args = p.parse_args()
    nk = args.heads if args.kv_heads is None else args.kv_heads
    if nk < 1 or args.heads % nk:
        p.error(f"--heads {args.heads} must be a multiple of --kv-heads {nk}")

    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group("nccl")
    else:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29744")
        dist.init_process_group("nccl", rank=0, world_size=1)
    rank = dist.get_rank()

    rows = []
    n, d = args.heads, 128
    if args.window:
        if world != 1:
            p.error("--window is a one-GPU measurement")
        windows = []
        for item in args.window:
            lr = [int(x) for x in item.split(",")]
            if len(lr) not in (1, 2) or min(lr) < -1:
                p.error("--window takes L or L,R with values >= -1")
            windows.append((lr[0], lr[1] if len(lr) == 2 else 0))
        dense = bench_burst(args, 1, args.seq, n, d, True, False, False,
                            args.steps, args.warmup, nk)
        rows.append(dense)
        for w in windows:
            rows.append(bench_window(args, args.seq, n, nk, d, w, dense,
                                     args.steps, args.warmup))
    elif args.configs == "quick":  # 1-GPU-friendly sweep
        for s in (16384, 32768, 65536):
            for causal in (False, True):
                rows.append(bench_burst(args, 1, s, n, d, causal, False, causal,
                                        args.steps, args.warmup, nk))
        if world == 1:
            rows.append(bench_single_flash(args, 1, 65536, n, d, False,
                                           args.steps, args.warmup))
    elif args.configs == "ring":  # the README seq sweep (per world size)
        for s in (65536, 131072, 262144, 524288):
            rows.append(bench_burst(args, 1, s, n, d, False, False, False,
                                    args.steps, args.warmup, nk))
        rows.append(bench_burst(args, 1, 524288, n, d, True, False, True,
                                args.steps, args.warmup, nk))  # config 4
    elif args.configs == "batch":  # README batch scaling at s=65536
        for b in (1, 2, 4, 8):
            rows.append(bench_burst(args, b, 65536, n, d, True, False, False,
                                    args.steps, args.warmup, nk))
    elif args.configs == "single":
        for s in (65536, 131072, 262144):
            rows.append(bench_single_flash(args, 1, s, n, d, False,
                                           args.steps, args.warmup))
    elif args.configs == "naive":  # RingQK/RingAV comparator column
        for s in (8192, 16384, 32768):
            r = bench_ring_naive(args, 1, s, n, d, args.steps, args.warmup)
            if r is not None:
                rows.append(r)
            r = bench_burst(args, 1, s, n, d, False, False, False,
                            args.steps, args.warmup)
            rows.append(r)
    elif args.configs == "gqa":  # equal-heads vs --kv-heads, and the
        # backward tile as group loop vs G-launch comparator
        for causal in (False, True):
            for h in dict.fromkeys((n, nk)):
                rows.append(bench_burst(args, 1, args.seq, n, d, causal, False,
                                        causal, args.steps, args.warmup, h))
            if world == 1:
                for g_launch in (False, True):
                    rows.append(bench_bwd_tile(args, 1, args.seq, n, nk, d,
                                               causal, g_launch, args.steps,
                                               args.warmup))

    elif args.configs == "packed":
        if world != 1:
            p.error("--configs packed is a one-GPU config")
        doc_lens = [int(x) for item in (args.doc_len or ["8192"])
                    for x in item.split(",")]
        if min(doc_lens) < 1:
            p.error("--doc-len must be positive")
        s = args.seq
        rows.append(bench_burst(args, 1, s, n, d, True, False, False,
                                args.steps, args.warmup, nk))
        if len(doc_lens) == 1 and s % doc_lens[0] == 0:
            rows.append(bench_burst(args, s // doc_lens[0], doc_lens[0], n, d,
                                    True, False, False, args.steps,
                                    args.warmup, nk))
        rows.append(bench_packed(args, s, n, nk, d, doc_lens, args.steps,
                                 args.warmup))
        for sp in (65536, 1048576):
            rows.append(bench_seg_prepass(args, sp, doc_lens[0], 20, 3))

    if rank == 0:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
                print(json.dumps(r), flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

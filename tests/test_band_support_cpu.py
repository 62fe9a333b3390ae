"""csrc/band_support.h, compiled by the host C++17 compiler and checked by
brute force against the element mask (no GPU, no HIP).

A small program includes the header and, for every (Sq, Sk, lo, hi) of the
sweep and every block index, compares ``ba_band_block_tiles`` with the set
of tiles that hold a visible pair, in both orientations (q-owning with the
band as given, kv-owning with ``ba_band_flip``), and the wave-level
predicates with the element mask.  The same program is built once more with
``-fsanitize=address,undefined`` and run on the clamped extremes: a plain
executable with its own ``main``.
"""

import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "burst_attn_amd", "csrc")

MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "band_support.h"

static long long fails = 0, checked = 0;
#define CHECK(c, ...) do { ++checked; if (!(c)) { if (fails++ < 20) { \
  printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// own side of S_own rows against streamed side of S_str rows, visible iff
// b.lo <= r - s <= b.hi
static void sweep(int S_own, int S_str, ba_band_args b, bool elements) {
  const int nblk = (S_own + BA_BAND_BLOCK - 1) / BA_BAND_BLOCK;
  const int ntile = (S_str + BA_BAND_TILE - 1) / BA_BAND_TILE;
  for (int blk = 0; blk < nblk; ++blk) {
    const ba_tile_range tr = ba_band_block_tiles(blk, b, S_own, S_str);
    CHECK(0 <= tr.lo && tr.lo <= tr.hi && tr.hi <= ntile, "range %d %d",
          tr.lo, tr.hi);
    int first = -1, last = -1;
    for (int t = 0; t < ntile; ++t) {
      // a tile holds a visible pair iff some streamed row s of it has an own
      // row r of the block with s + lo <= r <= s + hi
      bool vis = false;
      const long long r0 = (long long)blk * BA_BAND_BLOCK;
      const long long r1 = r0 + BA_BAND_BLOCK - 1 < S_own - 1
                               ? r0 + BA_BAND_BLOCK - 1 : S_own - 1;
      for (long long s = (long long)t * BA_BAND_TILE;
           s < (long long)(t + 1) * BA_BAND_TILE && s < S_str && !vis; ++s) {
        const long long a = s + b.lo > r0 ? s + b.lo : r0;
        const long long z = s + b.hi < r1 ? s + b.hi : r1;
        vis = a <= z;
      }
      if (vis) { if (first < 0) first = t; last = t; }
      if (vis) CHECK(tr.lo <= t && t < tr.hi, "blk %d tile %d outside [%d,%d) "
                     "S %d %d band %d %d", blk, t, tr.lo, tr.hi, S_own, S_str,
                     b.lo, b.hi);
    }
    if (first < 0)
      CHECK(tr.lo >= tr.hi, "blk %d: empty expected, got [%d,%d)", blk, tr.lo,
            tr.hi);
    else
      CHECK(tr.lo == first && tr.hi == last + 1,
            "blk %d: [%d,%d) expected [%d,%d) S %d %d band %d %d", blk, tr.lo,
            tr.hi, first, last + 1, S_own, S_str, b.lo, b.hi);
    if (!elements) continue;
    // wave level against the element mask (all 32 rows of the wave, also
    // those past S_own: the predicates do not know S_own)
    for (int w = 0; w < BA_BAND_BLOCK / BA_BAND_WAVE; ++w) {
      const int r0 = blk * BA_BAND_BLOCK + w * BA_BAND_WAVE;
      for (int t = 0; t < ntile; ++t) {
        const int s0 = t * BA_BAND_TILE;
        bool any = false, all = true;
        for (int r = r0; r < r0 + BA_BAND_WAVE; ++r)
          for (int s = s0; s < s0 + BA_BAND_TILE; ++s) {
            const bool v = ba_band_visible(r, s, b);
            any = any || v;
            all = all && v;
          }
        CHECK(ba_band_wave_active(r0, s0, b) == any, "active r0 %d s0 %d "
              "band %d %d", r0, s0, b.lo, b.hi);
        CHECK(ba_band_wave_inside(r0, s0, b) == all, "inside r0 %d s0 %d "
              "band %d %d", r0, s0, b.lo, b.hi);
      }
    }
  }
}

int main(int argc, char** argv) {
  if (argc == 6) {  // pairs lo hi S_own S_str
    printf("%lld\n", (long long)ba_band_tile_pairs(
        {atoi(argv[2]), atoi(argv[3])}, atoll(argv[4]), atoll(argv[5])));
    return 0;
  }
  const bool extremes_only = argc > 1;
  const int S[] = {1, 63, 64, 65, 255, 256, 257, 328, 600};
  std::vector<long long> bounds;
  if (!extremes_only)
    for (int x = -700; x <= 700; x += 37) bounds.push_back(x);
  bounds.push_back(-(1LL << 30));
  bounds.push_back(1LL << 30);
  // beyond the clamp: what a caller may hand the launcher
  const long long huge[] = {-(1LL << 62), 1LL << 62, -(1LL << 40), 1LL << 40};
  for (long long h : huge) {
    CHECK(ba_band_clamp(h) == (h < 0 ? -(1 << 30) : (1 << 30)), "clamp");
  }
  CHECK(ba_band_clamp(-5) == -5 && ba_band_clamp(7) == 7, "clamp identity");
  for (int sq : S)
    for (int sk : S)
      for (long long lo : bounds)
        for (long long hi : bounds) {
          if (lo > hi) continue;
          const ba_band_args b = {ba_band_clamp(lo), ba_band_clamp(hi)};
          // the wave predicates depend on row differences only: one
          // shape with several blocks and a ragged end covers them
          const bool el = sq == 328 && sk == 328;
          sweep(sq, sk, b, el);                 // forward, dq: own q
          sweep(sk, sq, ba_band_flip(b), el);   // dK/dV: own kv
        }
  // the largest lengths an int holds, at the clamped bounds: no overflow
  const ba_band_args wide = {-(1 << 30), 1 << 30};
  const long long big = 2147483647LL;
  const ba_tile_range r = ba_band_block_tiles((big - 1) / 256, wide, big, big);
  CHECK(r.lo <= r.hi && r.hi == (int)((big + 63) / 64), "big range %d %d",
        r.lo, r.hi);
  CHECK(ba_band_wave_active((int)(big - 32), 0, wide) == false, "big active");
  CHECK(ba_band_wave_active(0, (int)(big - 64), wide) == false, "big active 2");
  CHECK(ba_band_tile_pairs({0, 1 << 30}, 512, 512) == 4 + 8, "causal pairs");
  printf("checked %lld fails %lld\n", checked, fails);
  return fails ? 1 : 0;
}
"""


def _cc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which("c++"):
        return ["c++"]
    if shutil.which(hipcc):
        return [hipcc, "-x", "c++"]
    pytest.skip("no host C++ compiler")


def _build_and_run(tmp_path, flags, args):
    src, exe = tmp_path / "main.cpp", tmp_path / "main"
    src.write_text(MAIN)
    subprocess.run(_cc() + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC]
                   + flags + [str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)] + args, capture_output=True, text=True)


def test_band_ranges_and_wave_predicates_by_brute_force(tmp_path):
    r = _build_and_run(tmp_path, ["-O2"], [])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fails 0" in r.stdout


def test_no_overflow_at_the_clamped_bounds_under_sanitizers(tmp_path):
    """address + undefined-behaviour sanitizers on the stand-alone program,
    restricted to the clamped extremes (+-2^30) so that it stays quick."""
    r = _build_and_run(
        tmp_path, ["-O1", "-g", "-fsanitize=address,undefined",
                   "-fno-sanitize-recover=all"], ["extremes"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fails 0" in r.stdout and "runtime error" not in r.stderr


def test_sweep_script_counts_tile_pairs_like_the_header(tmp_path):
    """benchmarks/sweep.py restates ba_band_tile_pairs for its ideal ratio."""
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "sweep", os.path.join(CSRC, "..", "..", "benchmarks", "sweep.py"))
    sweep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sweep)
    for lo, hi, so, ss in ((0, 4096, 65536, 65536), (0, 1 << 30, 65536, 65536),
                           (-40, 70, 328, 328), (-250, -130, 96, 320),
                           (130, 250, 320, 96), (200, 400, 328, 328),
                           (5, 4, 328, 328)):
        r = _build_and_run(tmp_path, ["-O1"],
                           ["pairs", str(lo), str(hi), str(so), str(ss)])
        assert r.returncode == 0, r.stderr
        assert int(r.stdout) == sweep.band_tile_pairs(lo, hi, so, ss), (lo, hi)

// Host check of the planning of vecops_poly.hip (icicle_amd/csrc/poly_plan.h): a flat C surface for tests/test_poly_plan.py, which states
// the expected values in Python. With -DPOLY_PLAN_MAIN it is a stand-alone program that walks the same functions over a grid of shapes and
// simulates the tile schedule of the division on small integers modulo a prime (it is what runs under the sanitizers).
#include "../icicle_amd/csrc/poly_plan.h"
#include <cstdio>
#include <vector>
using namespace icicle_hip;

extern "C" int pp_tile(int words) { return poly_division_tile(words); }

// out = { split, chunk, chunks }
extern "C" void pp_eval_plan(uint64_t coeffs_size, uint64_t pairs, int key, uint64_t* out)
{
  const PolyEvalPlan p = poly_eval_plan(coeffs_size, pairs, key);
  out[0] = p.split, out[1] = p.chunk, out[2] = p.chunks;
}

// the levels of the split route as vecops_poly.hip walks them: out = chunk, chunks per level; returns the number of levels (0: point route)
extern "C" int pp_eval_levels(uint64_t coeffs_size, uint64_t pairs, int key, uint64_t* out, int max_levels)
{
  const PolyEvalPlan p = poly_eval_plan(coeffs_size, pairs, key);
  if (!p.split) return 0;
  uint64_t n = coeffs_size;
  for (int level = 0; level < max_levels; level++) {
    const uint64_t C = level == 0 ? p.chunk : poly_eval_chunk(n, pairs, key, false);
    const uint64_t chunks = (n + C - 1) / C;
    out[2 * level] = C, out[2 * level + 1] = chunks;
    if (chunks == 1) return level + 1;
    n = chunks;
  }
  return -1;
}

// out = { chunks, chunk_len }
extern "C" void pp_hnz_plan(uint64_t size, uint64_t* out)
{
  const PolyHnzPlan p = poly_hnz_plan(size);
  out[0] = p.chunks, out[1] = p.chunk_len;
}

extern "C" uint64_t pp_div_tiles(int64_t deg_n, int64_t deg_b, int64_t T) { return poly_division_tiles(deg_n, deg_b, T); }

// out = { hi, lo, cnt, nb, upd_lo, upd_cnt }; returns 1 where the entry has such a tile
extern "C" int pp_div_tile(int64_t deg_n, int64_t deg_b, int64_t T, int64_t tile, int64_t* out)
{
  PolyDivTile w;
  if (!poly_div_tile(deg_n, deg_b, T, tile, &w)) return 0;
  out[0] = w.hi, out[1] = w.lo, out[2] = w.cnt, out[3] = w.nb, out[4] = w.upd_lo, out[5] = w.upd_cnt;
  return 1;
}

// the argument rules; pointers are passed as plain numbers (0 = NULL)
extern "C" int pp_slice_check(int has_cfg, uint64_t in, int in_dev, uint64_t out, int out_dev, uint64_t offset, uint64_t stride, uint64_t size_in, uint64_t size_out,
                              uint64_t batch, uint64_t elem_bytes)
{
  return poly_slice_check(has_cfg != 0, (const void*)(uintptr_t)in, in_dev != 0, (const void*)(uintptr_t)out, out_dev != 0, offset, stride, size_in, size_out, batch, elem_bytes);
}
extern "C" int pp_hnz_check(int has_cfg, uint64_t in, uint64_t out, uint64_t size) { return poly_hnz_check(has_cfg != 0, (const void*)(uintptr_t)in, (const void*)(uintptr_t)out, size); }
extern "C" int pp_eval_check(int has_cfg, uint64_t coeffs, uint64_t domain, uint64_t evals, uint64_t coeffs_size, uint64_t domain_size, int key)
{
  return poly_eval_check(has_cfg != 0, (const void*)(uintptr_t)coeffs, (const void*)(uintptr_t)domain, (const void*)(uintptr_t)evals, coeffs_size, domain_size, key);
}
extern "C" int pp_division_check(int has_cfg, uint64_t num, uint64_t den, uint64_t q, uint64_t r, uint64_t num_size, int64_t den_size)
{
  return poly_division_check(has_cfg != 0, (const void*)(uintptr_t)num, (const void*)(uintptr_t)den, (const void*)(uintptr_t)q, (const void*)(uintptr_t)r, num_size, den_size);
}
extern "C" int pp_degree_check(int64_t deg_n, int64_t deg_b, uint64_t q_size, uint64_t r_size) { return poly_division_degree_check(deg_n, deg_b, q_size, r_size); }
extern "C" int pp_overlap(uint64_t a, uint64_t abytes, int a_dev, uint64_t b, uint64_t bbytes, int b_dev)
{
  return poly_overlap((const void*)(uintptr_t)a, abytes, a_dev != 0, (const void*)(uintptr_t)b, bbytes, b_dev != 0);
}

// The division as the two kernels perform it, tile by tile, over integers modulo P: every remainder coefficient must be touched by exactly
// the products the schedule assigns to it. Returns 0 when q * b + r == numerator, deg r < deg b and the window of every tile was left zero.
static const uint64_t P = 2013265921ull; // BabyBear
static uint64_t pw(uint64_t b, uint64_t e)
{
  uint64_t r = 1;
  for (; e; e >>= 1, b = b * b % P)
    if (e & 1) r = r * b % P;
  return r;
}
extern "C" int pp_div_simulate(const uint64_t* num, int64_t deg_n, const uint64_t* den, int64_t deg_b, int64_t T)
{
  if (deg_b < 0) return 1;
  std::vector<uint64_t> r(num, num + (deg_n + 1 > 0 ? deg_n + 1 : 0));
  const int64_t nq = deg_n - deg_b + 1;
  std::vector<uint64_t> q(nq > 0 ? nq : 0, 0);
  const uint64_t inv = pw(den[deg_b], P - 2);
  const uint64_t tiles = poly_division_tiles(deg_n, deg_b, T);
  for (uint64_t t = 0; t < tiles; t++) {
    PolyDivTile w;
    if (!poly_div_tile(deg_n, deg_b, T, (int64_t)t, &w)) return 2;
    if (w.cnt < 1 || w.cnt > T || w.nb != (deg_b + 1 < T ? deg_b + 1 : T)) return 3;
    // tile kernel: lane s owns r[deg_b + hi - s]
    for (int64_t step = 0; step < w.cnt; step++) {
      const uint64_t qv = r[deg_b + w.hi - step] * inv % P;
      q[w.hi - step] = qv;
      for (int64_t s = step + 1; s < w.cnt; s++) {
        const int64_t d = s - step;
        if (d < w.nb) r[deg_b + w.hi - s] = (r[deg_b + w.hi - s] + P - qv * den[deg_b - d] % P) % P;
      }
    }
    for (int64_t s = 0; s < w.cnt; s++)
      r[deg_b + w.hi - s] = 0;
    // update kernel
    for (int64_t i = w.upd_lo; i < w.upd_lo + w.upd_cnt; i++) {
      uint64_t acc = 0;
      for (int64_t s = 0; s < w.cnt; s++) {
        const int64_t bi = i - w.hi + s;
        if (bi >= 0 && bi <= deg_b) acc = (acc + q[w.hi - s] * den[bi]) % P;
      }
      r[i] = (r[i] + P - acc) % P;
    }
  }
  PolyDivTile past;
  if (poly_div_tile(deg_n, deg_b, T, (int64_t)tiles, &past)) return 4; // no tile beyond the last
  // q * den + r == num
  std::vector<uint64_t> back(r);
  for (int64_t m = 0; m < (int64_t)q.size(); m++)
    for (int64_t j = 0; j <= deg_b; j++)
      back[m + j] = (back[m + j] + q[m] * den[j]) % P;
  for (int64_t i = 0; i <= deg_n; i++)
    if (back[i] != num[i] % P) return 5;
  for (int64_t i = deg_b; i <= deg_n; i++)
    if (r[i] != 0) return 6;
  return 0;
}

#ifdef POLY_PLAN_MAIN
int main()
{
  uint64_t checksum = 0, out[100];
  int64_t tile_out[6];
  const int64_t T = poly_division_tile(1);
  // routes and levels
  for (uint64_t n : {1ull, 2ull, 63ull, 1024ull, 1025ull, 4097ull, 1ull << 20, (1ull << 24) + 5})
    for (uint64_t pairs : {1ull, 3ull, 64ull, 4096ull, 65472ull, 65473ull, 1ull << 20})
      for (int key : {-1, 0, 1, 2, 16, 64, 4096}) {
        pp_eval_plan(n, pairs, key, out);
        const int levels = pp_eval_levels(n, pairs, key, out + 3, 40);
        if (levels < 0) {
          printf("levels do not end: n %llu pairs %llu key %d\n", (unsigned long long)n, (unsigned long long)pairs, key);
          return 1;
        }
        checksum += out[0] + out[1] + out[2] + (uint64_t)levels;
      }
  for (uint64_t size : {1ull, 4096ull, 4097ull, 1ull << 22, (1ull << 22) + 1, 1ull << 40}) {
    pp_hnz_plan(size, out);
    if (out[0] * out[1] < size) return 2;
    checksum += out[0] + out[1];
  }
  // the tile schedule, simulated
  uint64_t seed = 12345;
  auto next = [&seed]() { return (seed = seed * 6364136223846793005ull + 1442695040888963407ull) >> 33; };
  for (int64_t tt : {(int64_t)4, T})
    for (int64_t nq : {(int64_t)1, tt - 1, tt, tt + 1, 2 * tt + 3})
      for (int64_t db : {(int64_t)0, (int64_t)1, tt - 1, tt, tt + 1}) {
        if (nq < 1) continue;
        const int64_t dn = db + nq - 1;
        std::vector<uint64_t> num(dn + 1), den(db + 1);
        for (auto& v : num)
          v = next() % P;
        for (auto& v : den)
          v = next() % P;
        if (num[dn] == 0) num[dn] = 1;
        if (den[db] == 0) den[db] = 1;
        if (nq > 3) num[dn - 1] = 0;
        const int rc = pp_div_simulate(num.data(), dn, den.data(), db, tt);
        if (rc) {
          printf("division schedule wrong: T %lld nq %lld deg_b %lld rc %d\n", (long long)tt, (long long)nq, (long long)db, rc);
          return 3;
        }
        for (int64_t t = 0; pp_div_tile(dn, db, tt, t, tile_out); t++)
          for (int k = 0; k < 6; k++)
            checksum += (uint64_t)tile_out[k];
      }
  // the argument rules
  for (int cfg = 0; cfg < 2; cfg++)
    for (uint64_t in : {0ull, 4096ull})
      for (uint64_t o : {0ull, 4096ull, 8192ull})
        for (uint64_t size_out : {0ull, 1ull, 5ull}) {
          checksum += (uint64_t)pp_slice_check(cfg, in, 1, o, 1, 3, 5, 24, size_out, 3, 4);
          checksum += (uint64_t)pp_hnz_check(cfg, in, o, size_out);
          checksum += (uint64_t)pp_eval_check(cfg, in, in, o, size_out, 4, (int)size_out - 2);
          checksum += (uint64_t)pp_division_check(cfg, in, in, o, o, size_out, (int64_t)size_out - 1);
        }
  checksum += (uint64_t)pp_degree_check(-1, -1, 0, 0) + (uint64_t)pp_degree_check(5, 2, 4, 6) + (uint64_t)pp_degree_check(5, 2, 3, 6) + (uint64_t)pp_degree_check(5, 2, 4, 5);
  checksum += (uint64_t)pp_slice_check(1, 4096, 1, 8192, 1, ~0ull, ~0ull, 24, ~0ull, 3, 4); // the bound in 128 bits
  printf("checksum %llu\n", (unsigned long long)checksum);
  return 0;
}
#endif

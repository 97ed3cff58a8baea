// Host-only planning of vecops_poly.hip: the argument rules of slice / highest_non_zero_idx / poly_eval / poly_division, the
// route and chunk length of poly_eval, the launch geometry of the degree scan and the tile schedule of the blocked division.
// No HIP in here: tests/poly_plan_harness.cpp compiles it with a plain host compiler (the tile schedule is also what the
// division kernels call on the device, hence POLY_HD).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
  #define POLY_HD __host__ __device__ inline
#else
  #define POLY_HD inline
#endif

namespace icicle_hip {

  // What an argument check says, in the order the entry points apply it (vector_inv's order): no config, then an empty call, then
  // a missing vector, then everything else.
  enum PolyCheck { POLY_OK = 0, POLY_EMPTY = 1, POLY_BAD_POINTER = 2, POLY_BAD_ARGUMENT = 3 };

  // do [a, a + abytes) and [b, b + bbytes) share a byte? Only buffers on the same side (both host or both device) are compared.
  inline bool poly_overlap(const void* a, uint64_t abytes, bool a_dev, const void* b, uint64_t bbytes, bool b_dev)
  {
    if (a_dev != b_dev || abytes == 0 || bbytes == 0) return false;
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return x < y + bbytes && y < x + abytes;
  }

  // a * b, saturating at 2^64 - 1
  inline uint64_t poly_mul_sat(uint64_t a, uint64_t b)
  {
    const unsigned __int128 m = (unsigned __int128)a * b;
    return m >> 64 ? ~0ull : (uint64_t)m;
  }

  // ---- slice: output[k][i] = input[k][offset + i * stride], i < size_out ----
  // size_out == 0 is an empty call; the last index read, offset + (size_out - 1) * stride, must lie below size_in (that covers
  // stride == 0 with an offset out of range); input and output must not overlap.
  inline PolyCheck poly_slice_check(bool has_cfg, const void* in, bool in_dev, const void* out, bool out_dev, uint64_t offset, uint64_t stride, uint64_t size_in,
                                    uint64_t size_out, uint64_t batch, uint64_t elem_bytes)
  {
    if (!has_cfg) return POLY_BAD_POINTER;
    if (size_out == 0) return POLY_EMPTY;
    if (!in || !out) return POLY_BAD_POINTER;
    const unsigned __int128 last = (unsigned __int128)offset + (unsigned __int128)(size_out - 1) * stride;
    if (last >= size_in) return POLY_BAD_ARGUMENT;
    if (poly_mul_sat(poly_mul_sat(size_in, batch), elem_bytes) >= (1ull << 56)) return POLY_BAD_ARGUMENT;
    if (poly_overlap(in, size_in * batch * elem_bytes, in_dev, out, size_out * batch * elem_bytes, out_dev)) return POLY_BAD_ARGUMENT;
    return POLY_OK;
  }

  // ---- highest_non_zero_idx: one int64 per batch entry ----
  inline PolyCheck poly_hnz_check(bool has_cfg, const void* in, const void* out, uint64_t size)
  {
    if (!has_cfg) return POLY_BAD_POINTER;
    if (!in || !out) return POLY_BAD_POINTER;
    if (size == 0 || size >= (1ull << 56)) return POLY_BAD_ARGUMENT;
    return POLY_OK;
  }

  // The scan is a max-reduction in the shape of reduce_run (vecops_tile.hpp): `chunks` blocks along an entry, each over chunk_len
  // elements, one partial per block, then a fold. A block of 256 lanes takes 16 elements per lane; beyond POLY_HNZ_MAX_CHUNKS blocks
  // per entry the chunks grow instead. The result is a maximum of exact integers: it does not depend on this geometry.
  constexpr uint64_t POLY_HNZ_PER_BLOCK = 4096;
  constexpr uint64_t POLY_HNZ_MAX_CHUNKS = 1024;
  struct PolyHnzPlan {
    uint32_t chunks = 1;
    uint64_t chunk_len = 0;
  };
  inline PolyHnzPlan poly_hnz_plan(uint64_t size)
  {
    PolyHnzPlan p;
    const uint64_t want = (size + POLY_HNZ_PER_BLOCK - 1) / POLY_HNZ_PER_BLOCK;
    p.chunks = (uint32_t)(want < 1 ? 1 : (want > POLY_HNZ_MAX_CHUNKS ? POLY_HNZ_MAX_CHUNKS : want));
    p.chunk_len = (size + p.chunks - 1) / p.chunks;
    return p;
  }

  // ---- poly_eval ----
  // chunk_key is config.ext "hip_poly_eval_chunk": 0 = the plan decides, positive = the split route with that chunk length, -1 = the
  // point route; any other negative value is an error. evals must overlap neither coeffs nor domain (the kernels read both while
  // other lanes already write).
  inline PolyCheck poly_eval_check(bool has_cfg, const void* coeffs, const void* domain, const void* evals, uint64_t coeffs_size, uint64_t domain_size, int chunk_key)
  {
    if (!has_cfg) return POLY_BAD_POINTER;
    if (!coeffs || !domain || !evals) return POLY_BAD_POINTER;
    if (coeffs_size == 0 || domain_size == 0 || chunk_key < -1) return POLY_BAD_ARGUMENT;
    if (coeffs_size >= (1ull << 48) || domain_size >= (1ull << 48)) return POLY_BAD_ARGUMENT;
    return POLY_OK;
  }

  // The two routes.
  //   point: one lane per (entry, point) runs Horner over all coefficients. It fills the machine when there are enough pairs.
  //   split: one WAVE per (entry, point, chunk of C coefficients): lane l runs Horner in x^64 over the coefficients l, l + 64, ... of
  //          its chunk, the 64 lane values are combined with x^1, x^2, x^4 ... x^32, and the chunk values form a polynomial in
  //          x^C that the next, much smaller, launch evaluates the same way, down to one chunk.
  // The threshold is a planning figure: each route has been timed far on its own side of it only, the threshold itself has NOT been
  // swept (profiles/poly_notes.md). The reasoning: an MI355X has 256 CUs of 4 SIMDs. The
  // point route is taken once its waves give every SIMD one wave (POLY_POINT_MIN_WAVES = 1024), however long the polynomial, and
  // for polynomials of at most POLY_SPLIT_MIN_COEFFS coefficients, where a second launch costs more than the Horner steps it saves
  // (a launch is a few microseconds, about a thousand dependent products). Below that the split route cuts the polynomial so that
  // pairs * chunks is about POLY_SPLIT_WAVES = 4096 waves (four per SIMD, enough to hide the latency of a dependent chain), in
  // chunks of a multiple of 64 and at least POLY_SPLIT_MIN_CHUNK = 256 coefficients (four steps per lane).
  constexpr uint64_t POLY_POINT_MIN_WAVES = 256 * 4;
  constexpr uint64_t POLY_SPLIT_WAVES = 256 * 4 * 4;
  constexpr uint64_t POLY_SPLIT_MIN_COEFFS = 1024;
  constexpr uint64_t POLY_SPLIT_MIN_CHUNK = 256;
  constexpr uint64_t POLY_SPLIT_FINAL_MAX = 4096; // a level of at most this many values is one chunk: the last launch

  struct PolyEvalPlan {
    bool split = false;
    uint64_t chunk = 0;  // C of the first level (split only)
    uint64_t chunks = 0; // ceil(coeffs_size / C)
  };

  // chunk length of one level of the split route: n values per pair, `first` for the level that reads the caller's coefficients
  inline uint64_t poly_eval_chunk(uint64_t n, uint64_t pairs, int chunk_key, bool first)
  {
    if (chunk_key > 0) return chunk_key < 2 ? 2 : (uint64_t)chunk_key; // a chunk of one coefficient would never shrink the polynomial
    if (!first && n <= POLY_SPLIT_FINAL_MAX) return n;
    const uint64_t want = pairs >= POLY_SPLIT_WAVES ? 1 : (POLY_SPLIT_WAVES + pairs - 1) / pairs;
    uint64_t c = (n + want - 1) / want;
    if (c < POLY_SPLIT_MIN_CHUNK) c = POLY_SPLIT_MIN_CHUNK;
    return (c + 63) / 64 * 64;
  }

  inline PolyEvalPlan poly_eval_plan(uint64_t coeffs_size, uint64_t pairs, int chunk_key)
  {
    PolyEvalPlan p;
    if (chunk_key == -1) return p;
    if (chunk_key == 0) {
      const uint64_t point_waves = (pairs + 63) / 64;
      if (point_waves >= POLY_POINT_MIN_WAVES || coeffs_size <= POLY_SPLIT_MIN_COEFFS) return p;
    }
    p.split = true;
    p.chunk = poly_eval_chunk(coeffs_size, pairs, chunk_key, true);
    p.chunks = (coeffs_size + p.chunk - 1) / p.chunk;
    return p;
  }

  // ---- poly_division: numerator = q * denominator + r per batch entry, blocked schoolbook ----
  // The quotient is produced from the top in tiles of POLY_DIV_TILE coefficients, two launches per tile: the tile kernel (one
  // workgroup per entry, one lane per quotient coefficient of the tile) and the update kernel over the rest of the remainder.
  constexpr int POLY_DIV_TILE = 256;
  inline int poly_division_tile(int words_per_element) { return (words_per_element == 1 || words_per_element == 2 || words_per_element == 8) ? POLY_DIV_TILE : 0; }

  inline PolyCheck poly_division_check(bool has_cfg, const void* num, const void* den, const void* q, const void* r, uint64_t num_size, int64_t den_size)
  {
    if (!has_cfg) return POLY_BAD_POINTER;
    if (!num || !den || !q || !r) return POLY_BAD_POINTER;
    if (num_size == 0 || den_size <= 0 || num_size >= (1ull << 48) || den_size >= (1ll << 48)) return POLY_BAD_ARGUMENT;
    return POLY_OK;
  }

  // the rules on the degrees of ONE entry (deg = highest_non_zero_idx, -1 for zero): a zero denominator, a remainder buffer that
  // cannot hold the numerator, a quotient buffer that cannot hold the quotient
  inline PolyCheck poly_division_degree_check(int64_t deg_n, int64_t deg_b, uint64_t q_size, uint64_t r_size)
  {
    if (deg_b < 0) return POLY_BAD_ARGUMENT;
    if ((int64_t)r_size < deg_n + 1) return POLY_BAD_ARGUMENT;
    const int64_t nq = deg_n - deg_b + 1;
    if (nq > 0 && (int64_t)q_size < nq) return POLY_BAD_ARGUMENT;
    return POLY_OK;
  }

  inline uint64_t poly_division_tiles(int64_t deg_n, int64_t deg_b, int64_t T)
  {
    const int64_t nq = deg_n - deg_b + 1;
    return (deg_b < 0 || nq <= 0) ? 0 : (uint64_t)((nq + T - 1) / T);
  }

  // Tile `tile` (0 = the top one) of an entry with nq = deg_n - deg_b + 1 quotient coefficients:
  //   the tile kernel produces q[lo .. hi], hi = nq - 1 - tile * T, from the remainder's window r[deg_b + lo .. deg_b + hi] and the top
  //   nb = min(T, deg_b + 1) coefficients of the denominator, and leaves that window zero;
  //   the update kernel then subtracts sum_m q[m] * b[i - m] from r[i] for i in [upd_lo, upd_lo + upd_cnt) = [lo, lo + deg_b).
  // Only the last tile can be partial (lo = 0). false: the entry has no such tile (nothing to divide, or all tiles done).
  struct PolyDivTile {
    int64_t hi, lo, cnt, nb, upd_lo, upd_cnt;
  };
  POLY_HD bool poly_div_tile(int64_t deg_n, int64_t deg_b, int64_t T, int64_t tile, PolyDivTile* w)
  {
    const int64_t nq = deg_n - deg_b + 1;
    if (deg_b < 0 || nq <= 0) return false;
    const int64_t hi = nq - 1 - tile * T;
    if (hi < 0) return false;
    const int64_t lo = hi - T + 1 < 0 ? 0 : hi - T + 1;
    w->hi = hi, w->lo = lo, w->cnt = hi - lo + 1;
    w->nb = deg_b + 1 < T ? deg_b + 1 : T;
    w->upd_lo = lo, w->upd_cnt = deg_b;
    return true;
  }

} // namespace icicle_hip

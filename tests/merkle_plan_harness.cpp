// Host check of the Merkle tree arithmetic (icicle_amd/csrc/merkle_plan.h, and the leaf-index arithmetic of merkle_batch.h): a flat
// C surface that tests/test_hash_cpu.py compares with the Python model (tests/merkle_model.py). With -DMERKLE_PLAN_MAIN it is a
// stand-alone program that walks a few shapes.
#include "../icicle_amd/csrc/merkle_batch.h"
#include <cstdio>
using namespace icicle_hip;

// out = { capacity, full path, pruned path, n_0 .. n_{L-1} }; returns 0, or 1 where the layers are no tree
extern "C" int mp_plan(const uint64_t* chunk, const uint64_t* outsz, int L, uint64_t es, uint64_t* out)
{
  MerklePlan p;
  if (!merkle_make_plan(chunk, outsz, L, es, &p)) return 1;
  out[0] = p.capacity, out[1] = p.full_path, out[2] = p.pruned_path;
  for (int i = 0; i < L; i++)
    out[3 + i] = p.layers[i].count;
  return 0;
}

// out = { full_chunks, pad_bytes, last_off }; returns 0, 1 = invalid argument, 2 = no tree
extern "C" int mp_padding(const uint64_t* chunk, const uint64_t* outsz, int L, uint64_t es, uint64_t leaves_size, int policy, uint64_t* out)
{
  MerklePlan p;
  if (!merkle_make_plan(chunk, outsz, L, es, &p)) return 2;
  MerklePadding pad;
  if (merkle_padding(p, leaves_size, policy, &pad)) return 1;
  out[0] = pad.full_chunks, out[1] = pad.pad_bytes, out[2] = pad.last_off;
  return 0;
}

// out = { chunk0, path size, sub_first, sub_count, then per layer 0 .. L-2: node, src_off, len, skip_off, dst_off,
//         then the L-1 offsets verify() walks for a leaf of c_0 bytes }
extern "C" int mp_proof(const uint64_t* chunk, const uint64_t* outsz, int L, uint64_t es, uint64_t leaf_idx, int pruned, int store_min, uint64_t* out)
{
  MerklePlan p;
  if (!merkle_make_plan(chunk, outsz, L, es, &p)) return 2;
  MerkleBatchShape sh;
  merkle_batch_shape(p, pruned != 0, store_min, &sh);
  if (!merkle_batch_chunk0(sh, leaf_idx, &out[0])) return 1;
  out[1] = merkle_batch_path_size(sh);
  merkle_batch_subtree(sh, out[0], &out[2], &out[3]);
  uint64_t* o = out + 4;
  for (int l = 0; l < sh.steps; l++) {
    MerkleBatchStep s;
    merkle_batch_step(sh, out[0], l, &s);
    *o++ = s.node, *o++ = s.src_off, *o++ = s.len, *o++ = s.skip_off, *o++ = s.dst_off;
  }
  std::vector<uint64_t> offs;
  merkle_verify_offsets(p, leaf_idx, p.layers[0].chunk, &offs);
  for (uint64_t v : offs)
    *o++ = v;
  return 0;
}

#ifdef MERKLE_PLAN_MAIN
int main()
{
  struct Shape {
    std::vector<uint64_t> chunk, out;
    uint64_t es;
  };
  const Shape shapes[] = {{{64, 64, 64, 64, 64}, {32, 32, 32, 32, 32}, 32},
                          {{100, 256, 128, 64}, {64, 32, 32, 64}, 20},
                          {{1000}, {32}, 8},
                          {{96, 96, 96}, {32, 32, 32}, 32},
                          {{64, 96}, {64, 64}, 32}};
  uint64_t checksum = 0;
  for (const Shape& s : shapes) {
    const int L = (int)s.chunk.size();
    std::vector<uint64_t> out(8 + 8 * L);
    if (mp_plan(s.chunk.data(), s.out.data(), L, s.es, out.data())) {
      printf("no tree (%d layers)\n", L);
      continue;
    }
    const uint64_t cap = out[0];
    printf("L %d capacity %llu full %llu pruned %llu\n", L, (unsigned long long)cap, (unsigned long long)out[1], (unsigned long long)out[2]);
    for (int policy = 0; policy < 4; policy++)
      for (uint64_t size : {(uint64_t)0, (uint64_t)1, s.es, cap / 3, cap - s.es, cap, cap + 1})
        if (mp_padding(s.chunk.data(), s.out.data(), L, s.es, size, policy, out.data()) == 0) checksum += out[0] + out[1] + out[2];
    for (uint64_t idx = 0; idx <= cap / s.es + 1; idx++)
      for (int pruned = 0; pruned < 2; pruned++)
        for (int m = 0; m <= L; m++)
          if (mp_proof(s.chunk.data(), s.out.data(), L, s.es, idx, pruned, m, out.data()) == 0)
            for (int k = 0; k < 4 + 6 * (L - 1); k++)
              checksum += out[k];
  }
  printf("checksum %llu\n", (unsigned long long)checksum);
  return 0;
}
#endif

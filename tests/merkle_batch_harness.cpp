// Test infrastructure: a stand-alone program over icicle_amd/csrc/merkle_batch.h (no HIP), compiled with g++ by
// tests/test_merkle_batch_cpu.py -- once plainly and once with -fsanitize=address,undefined. It holds the index function the gather
// kernel and the host's unpacking share -- the product's only leaf-index arithmetic -- against the straightforward loop form of
// the same walk (ref_proof_plan below, test-only reference code) for EVERY leaf index of small trees, pruned and full, for every
// choice of the first stored layer, and checks the staging record: pieces in order, 16-aligned, without overlap, covering the
// stride, and found again by merkle_batch_piece from every byte offset. Prints one line per tree and "ok <trees>".
#include "../icicle_amd/csrc/merkle_batch.h"
#include <cstdio>
#include <cstdlib>
using namespace icicle_hip;

// ---- the reference: one walk from the leaf to the root over the MerklePlan, all layers at once --------------------------------------
// One layer's share of a proof's path (reference: icicle/backend/cpu/src/hash/cpu_merkle_tree.cpp:546-573): the a_{i+1} digests of
// layer i that form the one input of layer i + 1 on the way from the leaf to the root. Pruned, the digest ON the way is left out.
struct RefProofStep {
  uint64_t node = 0;     // index of the on-path digest in layer i
  uint64_t src_off = 0;  // byte offset of the group in layer i's digests
  uint64_t len = 0;      // c_{i+1}
  uint64_t skip_off = 0; // byte offset of the on-path digest inside the group
  uint64_t dst_off = 0;  // where the group starts in the path
};
struct RefProofPlan {
  uint64_t chunk0 = 0;             // the layer-0 chunk that holds the element; the proof's leaf is this whole chunk
  std::vector<RefProofStep> steps; // layers 0 .. L-2
  uint64_t path_size = 0;
  // layers below output_store_min_layer are not kept: the proof re-hashes the sub-tree under the on-path node of layer
  // store_min -- layer-0 chunks [sub_first, sub_first + sub_count), and n_i / n_store_min nodes of every layer i below it,
  // the first of them node sub_first * n_i / n_0
  uint64_t sub_first = 0, sub_count = 0;
};
// 0 = fine, 1 = leaf_idx * leaf_element_size lies at or beyond the capacity
static int ref_proof_plan(const MerklePlan& p, uint64_t leaf_idx, bool pruned, int store_min, RefProofPlan* out)
{
  const int L = p.L();
  if (leaf_idx >= p.capacity / p.leaf_element_size + 1) return 1;
  const uint64_t byte0 = leaf_idx * p.leaf_element_size;
  if (byte0 >= p.capacity) return 1;
  out->chunk0 = byte0 / p.layers[0].chunk;
  out->steps.assign(L > 0 ? L - 1 : 0, RefProofStep{});
  uint64_t node = out->chunk0, dst = 0;
  for (int i = 0; i + 1 < L; i++) {
    const uint64_t a = p.arity(i + 1), o = p.layers[i].out;
    RefProofStep& s = out->steps[i];
    s.node = node;
    s.src_off = (node / a) * a * o;
    s.len = p.layers[i + 1].chunk;
    s.skip_off = (node % a) * o;
    s.dst_off = dst;
    dst += pruned ? s.len - o : s.len;
    node /= a;
  }
  out->path_size = dst;
  if (store_min < 0) store_min = 0;
  if (store_min > L - 1) store_min = L - 1;
  out->sub_count = p.layers[0].count / p.layers[store_min].count;
  out->sub_first = (out->chunk0 / out->sub_count) * out->sub_count;
  return 0;
}

static int g_failures = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (g_failures++ < 20) {                                                                                         \
        printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);                                                          \
        printf(__VA_ARGS__);                                                                                           \
        printf("\n");                                                                                                  \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)

static void check_layout(const MerkleBatchShape& s)
{
  // the pieces in order: groups of layers 0 .. steps-1, the leaf chunk, the last element
  std::vector<uint64_t> at, len;
  for (int i = 0; i < s.steps; i++)
    at.push_back(s.stage_at[i]), len.push_back(s.len[i]);
  at.push_back(s.leaf_at), len.push_back(s.c0);
  at.push_back(s.last_at), len.push_back(s.es);
  uint64_t expect = 0;
  for (size_t k = 0; k < at.size(); k++) {
    CHECK(at[k] == expect, "piece %zu at %llu, expected %llu", k, (unsigned long long)at[k], (unsigned long long)expect);
    CHECK(at[k] % 16 == 0, "piece %zu not 16-aligned", k);
    CHECK(len[k] > 0, "piece %zu empty", k);
    expect = at[k] + merkle_batch_pad16(len[k]); // no overlap: the next piece starts behind this one's padded end
  }
  CHECK(expect == s.stride, "pieces end at %llu, stride %llu", (unsigned long long)expect, (unsigned long long)s.stride);
  CHECK(s.stride % 16 == 0, "stride");
  // every byte of the record belongs to exactly the piece the walk above puts it in, or to a piece's padding
  std::vector<int> owner(s.stride, -1);
  for (size_t k = 0; k < at.size(); k++)
    for (uint64_t b = 0; b < len[k]; b++) {
      CHECK(owner[at[k] + b] == -1, "byte %llu owned twice", (unsigned long long)(at[k] + b));
      owner[at[k] + b] = (int)k;
    }
  for (uint64_t off = 0; off < s.stride; off++) {
    uint64_t q = ~0ull, n = ~0ull;
    const int piece = merkle_batch_piece(s, off, &q, &n);
    CHECK(piece == owner[off], "offset %llu: piece %d, expected %d", (unsigned long long)off, piece, owner[off]);
    if (piece >= 0) CHECK(q == off - at[piece] && n == len[piece], "offset %llu: q %llu len %llu", (unsigned long long)off, (unsigned long long)q, (unsigned long long)n);
  }
}

static uint64_t check_tree(const std::vector<uint64_t>& chunk, const std::vector<uint64_t>& out, uint64_t es)
{
  const int L = (int)chunk.size();
  MerklePlan p;
  if (!merkle_make_plan(chunk.data(), out.data(), L, es, &p)) {
    CHECK(false, "no tree");
    return 0;
  }
  uint64_t checked = 0;
  for (int store_min : {0, 1, L - 1, L + 3})
    for (int pruned = 0; pruned < 2; pruned++) {
      MerkleBatchShape s;
      merkle_batch_shape(p, pruned != 0, store_min, &s);
      CHECK(s.steps == L - 1, "steps");
      check_layout(s);
      CHECK(merkle_batch_path_size(s) == (pruned ? p.pruned_path : p.full_path), "path size");
      // every index the tree has, and a few it has not
      for (uint64_t idx = 0; idx <= p.capacity / es + 2; idx++) {
        RefProofPlan pp;
        const int refused = ref_proof_plan(p, idx, pruned != 0, store_min, &pp);
        uint64_t chunk0 = ~0ull;
        const bool ok = merkle_batch_chunk0(s, idx, &chunk0);
        CHECK(ok == !refused, "index %llu: accepted %d, plan refuses %d", (unsigned long long)idx, ok, refused);
        if (!ok || refused) continue;
        CHECK(chunk0 == pp.chunk0, "index %llu: chunk0", (unsigned long long)idx);
        uint64_t first = ~0ull, count = ~0ull;
        merkle_batch_subtree(s, chunk0, &first, &count);
        CHECK(first == pp.sub_first && count == pp.sub_count, "index %llu: sub-tree %llu+%llu, plan %llu+%llu", (unsigned long long)idx, (unsigned long long)first,
              (unsigned long long)count, (unsigned long long)pp.sub_first, (unsigned long long)pp.sub_count);
        CHECK(merkle_batch_path_size(s) == pp.path_size, "index %llu: path size", (unsigned long long)idx);
        for (int l = 0; l + 1 < L; l++) {
          MerkleBatchStep st;
          merkle_batch_step(s, chunk0, l, &st);
          const RefProofStep& w = pp.steps[l];
          CHECK(st.node == w.node && st.src_off == w.src_off && st.len == w.len && st.skip_off == w.skip_off && st.dst_off == w.dst_off, "index %llu layer %d pruned %d",
                (unsigned long long)idx, l, pruned);
          // where the group lies in the re-hashed sub-tree: relative to the layer's first node under the sub-tree's root, i.e.
          // node sub_first / (layer-0 chunks per node of the layer); the whole group inside the sub-tree's share of the layer
          const int m = s.store_min;
          if (l < m) {
            const uint64_t ratio = p.layers[0].count / p.layers[l].count, node0 = pp.sub_first / ratio, nodes = pp.sub_count / ratio;
            CHECK(st.sub_off == w.src_off - node0 * p.layers[l].out, "index %llu layer %d: sub_off", (unsigned long long)idx, l);
            CHECK(st.sub_off + st.len <= nodes * p.layers[l].out, "index %llu layer %d: group leaves the sub-tree", (unsigned long long)idx, l);
          } else {
            CHECK(st.sub_off == w.src_off, "index %llu layer %d: stored layer", (unsigned long long)idx, l);
            CHECK(st.src_off + st.len <= p.layers[l].count * p.layers[l].out, "index %llu layer %d: group leaves the layer", (unsigned long long)idx, l);
          }
          checked++;
        }
        checked++;
      }
    }
  printf("L %d es %llu capacity %llu checked %llu\n", L, (unsigned long long)es, (unsigned long long)p.capacity, (unsigned long long)checked);
  return checked;
}

int main()
{
  int trees = 0;
  // arity 2 and 4 (and both in one tree), a leaf chunk of 1 and of 4 elements, 32- and 64-byte digests mixed, 1, 2 and 6 layers
  for (uint64_t per_chunk : {1, 4}) {
    const uint64_t es = 4, c0 = es * per_chunk;
    check_tree({c0}, {32}, es), trees++;
    check_tree({c0}, {64}, es), trees++;
    check_tree({c0, 64}, {32, 32}, es), trees++;        // arity 2
    check_tree({c0, 256}, {64, 32}, es), trees++;       // arity 4 over 64-byte digests
    check_tree({c0, 64, 64, 64, 64, 64}, {32, 32, 32, 32, 32, 32}, es), trees++;
    check_tree({c0, 128, 128, 128, 128, 128}, {32, 32, 32, 32, 32, 32}, es), trees++; // arity 4
    check_tree({c0, 128, 64, 256, 128, 64}, {64, 32, 64, 64, 32, 64}, es), trees++; // digests and arities mixed: 2, 2, 4, 2, 2
  }
  check_tree({20, 96, 96}, {32, 32, 32}, 20), trees++; // arity 3, an element size that is no power of two
  if (g_failures) {
    printf("%d failures\n", g_failures);
    return 1;
  }
  printf("ok %d\n", trees);
  return 0;
}

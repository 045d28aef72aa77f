// Exact k-nearest-neighbour search by squared L2 distance: Q float32 query rows against the N rows of a table (uint8, an element meaning
// byte_to_unit(v), or float32) of D elements each -> per query the k rows of least (distance, row index), ascending. Evaluation only.
//
// The distance is sum_i (q_i - t_i)^2 with the difference taken first (one subtract, one fma per pair-element, never the expansion
// |q|^2 + |t|^2 - 2 q.t, which loses a near-duplicate's distance to cancellation) and ONE summation order per D: elements in chunks of
// kNnKC, a chunk's squares accumulated in element order from zero, the chunk sums added in chunk order. Elements past D are staged as
// zeros in both operands, and x + 0 == x, so a pair's bits depend on the two rows and D alone: not on Q, N, k, exclude, the position or
// alignment of either row, or how the launch is cut. Tiles are staged with element loads of any alignment.
//
// Launch 1 (pairs): a workgroup of 256 threads owns kNnTQ queries and a run of consecutive slabs of kNnTN table rows. Per slab it stages
// D-chunks of both tiles in LDS element-major (uint8 converted once per staged element through a 256-entry table of byte_to_unit), each
// thread accumulating a 4 x 4 register tile of pairs over the whole of D (packed fp32 subtract and fma, two rows per instruction, LDS reads
// issued two elements ahead of their use); the slab's distances then go to LDS as keys and are merged into
// the workgroup's running k best per query by counting ranks (the keys of a query are distinct: ties fall to the lower row). The run's
// k best go to the workspace as [Q][groups][k] 64-bit keys (distance bits, row). Launch 2 (merge): one workgroup per query takes the k
// least keys of its groups, one block-wide minimum per output slot. No float atomics, no host wait.
//
// Key of a distance: its bits (distances are >= +0, so bit order is value order, +inf above every finite value), every NaN as 0x7fc00000
// (above +inf); 0xffffffff marks a slot without an eligible row, which comes out as (-1, +inf).
#include "lvae_host.h"

namespace lvae {

constexpr int kNnTQ = 32;             // queries per workgroup
constexpr int kNnTN = 128;            // table rows per slab
constexpr int kNnKC = 32;             // elements per staged chunk: the unit of the summation order
constexpr int kNnQS = kNnTQ + 4;      // LDS row strides in floats: 16-byte aligned rows, element-major
constexpr int kNnTS = kNnTN + 4;
constexpr int kNnMaxK = 32;
constexpr int kNnLS = kNnMaxK + 1;    // stride of a query's running list
constexpr int kNnGroups = 512;        // workgroups the pair launch aims for (two per CU), at least kNnMinGroups row groups per query tile
constexpr int kNnMinGroups = 8;
constexpr uint32_t kNnNone = 0xffffffffu;
constexpr uint32_t kNnNan = 0x7fc00000u;

struct NnPairArgs {
  const float* queries;        // [Q][D]
  const void* table;           // [N][D] uint8 or float32
  const int32_t* exclude;      // [Q] or null
  unsigned long long* cand;    // [Q][groups][k]
  int64_t N, D;
  int Q, k, slabs, per_group, groups;
};

struct NnMergeArgs {
  const unsigned long long* cand;
  int groups, k;
  int32_t* index_out;          // [Q][k]
  float* dist_out;             // [Q][k]
};

__device__ __forceinline__ uint32_t nn_key(float d) { return d != d ? kNnNan : __float_as_uint(d); }

// groups of consecutive slabs a query tile's rows are cut into, and slabs per group (host)
static void nn_cut(int32_t Q, int64_t N, int& qtiles, int& slabs, int& per_group, int& groups) {
  qtiles = (int)(((int64_t)Q + kNnTQ - 1) / kNnTQ);
  slabs = (int)((N + kNnTN - 1) / kNnTN);
  int want = (kNnGroups + qtiles - 1) / qtiles;
  if (want < kNnMinGroups) want = kNnMinGroups;
  if (want > slabs) want = slabs;
  per_group = (slabs + want - 1) / want;
  groups = (slabs + per_group - 1) / per_group;
}

template <bool F32>
__global__ __launch_bounds__(256) void nn_pairs_kernel(NnPairArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kNnKC * (kNnQS + kNnTS)];  // query chunk, table chunk; then the slab's distance keys
  __shared__ uint32_t list_d[kNnTQ * kNnLS], list_i[kNnTQ * kNnLS];             // running k best per query, ascending
  __shared__ float unit[256];
  float* qs = tile;
  float* ts = tile + kNnKC * kNnQS;
  uint32_t* nd = reinterpret_cast<uint32_t*>(tile);  // [kNnTQ][kNnTS]

  const int tid = threadIdx.x;
  const int qt = blockIdx.x / a.groups, g = blockIdx.x - qt * a.groups;
  const int64_t q0 = (int64_t)qt * kNnTQ;
  const int tq = tid >> 5, tr = tid & 31;       // register tile: queries 4 tq .. + 3, rows 4 tr .. + 3
  const int se = tid & 31, sr = tid >> 5;       // staging: element se of rows sr, sr + 8, ...
  const int rq = tid >> 3, sub = tid & 7;       // ranking: query rq, entries sub, sub + 8, ...

  unit[tid] = byte_to_unit((unsigned)tid);
  for (int e = tid; e < kNnTQ * kNnLS; e += 256) list_d[e] = kNnNone, list_i[e] = kNnNone;
  int32_t excl[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t qi = q0 + tq * 4 + u;
    excl[u] = (a.exclude != nullptr && qi < a.Q) ? a.exclude[qi] : -1;
  }
  __syncthreads();
  const float* tf = static_cast<const float*>(a.table);
  const unsigned char* tb = static_cast<const unsigned char*>(a.table);

  const int s_end = min(a.slabs, (g + 1) * a.per_group);
  for (int s = g * a.per_group; s < s_end; ++s) {
    const int64_t r0 = (int64_t)s * kNnTN;
    float acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;

    // a chunk's elements in registers: plain element loads (any alignment), zeros past D, N and Q. Loaded one chunk ahead of the LDS copy.
    float qv[kNnTQ / 8], tv[kNnTN / 8];
    unsigned bv[kNnTN / 8];
    auto load_chunk = [&](int64_t i0) {
      const int64_t i = i0 + se;
      const bool iin = i < a.D;
#pragma unroll
      for (int p = 0; p < kNnTQ / 8; ++p) {
        const int64_t qi = q0 + sr + 8 * p;
        qv[p] = (iin && qi < a.Q) ? a.queries[qi * a.D + i] : 0.f;
      }
#pragma unroll
      for (int p = 0; p < kNnTN / 8; ++p) {
        const int64_t ri = r0 + sr + 8 * p;
        const bool in = iin && ri < a.N;
        if (F32) tv[p] = in ? tf[ri * a.D + i] : 0.f;
        else bv[p] = in ? (unsigned)tb[ri * a.D + i] : 0u;
      }
    };
    load_chunk(0);
    for (int64_t i0 = 0; i0 < a.D; i0 += kNnKC) {
      __syncthreads();  // the previous chunk (or the previous slab's keys) is no longer read
#pragma unroll
      for (int p = 0; p < kNnTQ / 8; ++p) qs[se * kNnQS + sr + 8 * p] = qv[p];
#pragma unroll
      for (int p = 0; p < kNnTN / 8; ++p) ts[se * kNnTS + sr + 8 * p] = F32 ? tv[p] : unit[bv[p]];
      __syncthreads();
      if (i0 + kNnKC < a.D) load_chunk(i0 + kNnKC);

      // two rows per instruction: packed fp32 subtract and fma (each half an IEEE operation, the same bits as the scalar pair)
      f32x2 part[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) part[u][0] = part[u][1] = f32x2{0.f, 0.f};
      // the LDS reads of element e + 2 are issued before element e is summed: two waves per SIMD do not hide an LDS round trip
      f32x4 xr[3], yr[3];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        xr[e] = *reinterpret_cast<const f32x4*>(qs + e * kNnQS + tq * 4);
        yr[e] = *reinterpret_cast<const f32x4*>(ts + e * kNnTS + tr * 4);
      }
#pragma unroll
      for (int e = 0; e < kNnKC; ++e) {
        if (e + 2 < kNnKC) {
          xr[(e + 2) % 3] = *reinterpret_cast<const f32x4*>(qs + (e + 2) * kNnQS + tq * 4);
          yr[(e + 2) % 3] = *reinterpret_cast<const f32x4*>(ts + (e + 2) * kNnTS + tr * 4);
        }
        const f32x4 x = xr[e % 3], y = yr[e % 3];
        const f32x2 y01{y[0], y[1]}, y23{y[2], y[3]};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f32x2 xx{x[u], x[u]};
          const f32x2 d0 = xx - y01, d1 = xx - y23;
          part[u][0] = __builtin_elementwise_fma(d0, d0, part[u][0]);
          part[u][1] = __builtin_elementwise_fma(d1, d1, part[u][1]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += part[u][v >> 1][v & 1];
    }

    // the slab's keys: a row outside the table, a query outside the batch and the excluded row are not eligible
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t qi = q0 + tq * 4 + u, ri = r0 + tr * 4 + v;
        const bool ok = qi < a.Q && ri < a.N && ri != (int64_t)excl[u];
        nd[(tq * 4 + u) * kNnTS + tr * 4 + v] = ok ? nn_key(acc[u][v]) : kNnNone;
      }
    __syncthreads();

    // ranks in the union of the running list (rows below this slab: they win ties) and the slab. An entry at or above the list's k-th key
    // cannot place; one below it counts the keys before it.
    const uint32_t* mine = nd + rq * kNnTS;
    const uint32_t* ld = list_d + rq * kNnLS;
    const uint32_t kth = ld[a.k - 1];
    uint32_t new_d[kNnTN / 8];
    int new_r[kNnTN / 8];
#pragma unroll
    for (int j = 0; j < kNnTN / 8; ++j) {
      const int c = sub + 8 * j;
      const uint32_t d = mine[c];
      int r = kNnMaxK;
      if (d < kth) {  // (kNnNone is never below anything)
        r = 0;
        for (int m = 0; m < a.k; ++m) r += ld[m] <= d;
#pragma unroll 4
        for (int o = 0; o < kNnTN; ++o) {
          const uint32_t w = mine[o];
          r += (w < d) || (w == d && o < c);
        }
      }
      new_d[j] = d, new_r[j] = r;
    }
    uint32_t old_d[kNnMaxK / 8], old_i[kNnMaxK / 8];
    int old_r[kNnMaxK / 8];
#pragma unroll
    for (int j = 0; j < kNnMaxK / 8; ++j) {
      const int m = sub + 8 * j;
      const uint32_t d = ld[m];
      int r = kNnMaxK;
      if (m < a.k && d != kNnNone) {
        r = m;
#pragma unroll 4
        for (int o = 0; o < kNnTN; ++o) r += mine[o] < d;
      }
      old_d[j] = d, old_i[j] = list_i[rq * kNnLS + m], old_r[j] = r;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kNnTN / 8; ++j)
      if (new_r[j] < a.k) {
        list_d[rq * kNnLS + new_r[j]] = new_d[j];
        list_i[rq * kNnLS + new_r[j]] = (uint32_t)(r0 + sub + 8 * j);
      }
#pragma unroll
    for (int j = 0; j < kNnMaxK / 8; ++j)
      if (old_r[j] < a.k) {
        list_d[rq * kNnLS + old_r[j]] = old_d[j];
        list_i[rq * kNnLS + old_r[j]] = old_i[j];
      }
    // (the next slab's first barrier, or the one below, orders these writes before the next read)
  }
  __syncthreads();
  for (int e = tid; e < kNnTQ * a.k; e += 256) {
    const int ql = e / a.k, m = e - ql * a.k;
    const int64_t qi = q0 + ql;
    if (qi >= a.Q) continue;
    const uint32_t d = list_d[ql * kNnLS + m];
    a.cand[((size_t)qi * a.groups + g) * a.k + m] = ((unsigned long long)d << 32) | list_i[ql * kNnLS + m];
  }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(NnMergeArgs a) {
  __shared__ unsigned long long red[4];
  const int tid = threadIdx.x;
  const unsigned long long* c = a.cand + (size_t)blockIdx.x * a.groups * a.k;
  const int n = a.groups * a.k;
  const unsigned long long none = ~0ull;
  unsigned long long prev = 0;
  for (int r = 0; r < a.k; ++r) {
    unsigned long long best = none;
    for (int e = tid; e < n; e += 256) {
      const unsigned long long v = c[e];
      if ((r == 0 || v > prev) && v < best) best = v;  // valid keys are distinct (their rows are)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long w = __shfl_xor(best, o, 64);
      best = w < best ? w : best;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = red[w] < best ? red[w] : best;
    if (tid == 0) {
      const size_t o = (size_t)blockIdx.x * a.k + r;
      a.index_out[o] = best == none ? -1 : (int32_t)(uint32_t)best;
      a.dist_out[o] = best == none ? __uint_as_float(0x7f800000u) : __uint_as_float((uint32_t)(best >> 32));
    }
    prev = best;  // once `none`, nothing is above it: every later slot is `none` too
  }
}

}  // namespace lvae

using namespace lvae;

// [Q][groups][k] keys, bounded by an expression that grows with each of Q, N and k (the cut itself does not: more query tiles mean
// fewer groups): groups <= slabs, and groups <= max(kNnMinGroups, kNnGroups / qtiles + 1).
extern "C" size_t lvae_nn_l2_workspace(int32_t Q, int64_t N, int32_t k) {
  if (Q < 1 || N < 1 || N > INT32_MAX || k < 1 || k > kNnMaxK) return 0;
  const size_t qtiles = ((size_t)Q + kNnTQ - 1) / kNnTQ, qpad = qtiles * kNnTQ;
  const size_t slabs = ((size_t)N + kNnTN - 1) / kNnTN;
  size_t rows = qpad * kNnMinGroups;
  if (rows < (size_t)kNnGroups * kNnTQ + qpad) rows = (size_t)kNnGroups * kNnTQ + qpad;
  if (rows > qpad * slabs) rows = qpad * slabs;
  return rows * (size_t)k * sizeof(unsigned long long);
}

extern "C" int lvae_nn_l2_f32(const float* queries, int32_t Q, const void* table, int32_t table_kind, int64_t N, int64_t D,
                              const int32_t* exclude, int32_t k, int32_t* index_out, float* dist_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
  LVAE_REQUIRE(queries && table && index_out && dist_out, LVAE_EINVAL, "lvae_nn_l2_f32: queries, table, index_out or dist_out missing");
  LVAE_REQUIRE(table_kind == LVAE_FEED_U8 || table_kind == LVAE_FEED_F32, LVAE_EINVAL, "lvae_nn_l2_f32: table kind %d is neither uint8 nor float32",
               (int)table_kind);
  LVAE_REQUIRE(Q >= 1 && N >= 1 && N <= INT32_MAX && D >= 1 && k >= 1 && k <= kNnMaxK, LVAE_EINVAL,
               "lvae_nn_l2_f32: Q %d, N %lld, D %lld, k %d (1 <= k <= %d, N <= INT32_MAX)", (int)Q, (long long)N, (long long)D, (int)k, kNnMaxK);
  LVAE_REQUIRE((int64_t)Q * k <= INT32_MAX && D <= (INT64_MAX >> 3) / N && D <= (INT64_MAX >> 3) / Q, LVAE_EINVAL,
               "lvae_nn_l2_f32: %d x %d results or %lld rows of %lld elements exceed the index ranges", (int)Q, (int)k, (long long)N, (long long)D);
  int qtiles, slabs, per_group, groups;
  nn_cut(Q, N, qtiles, slabs, per_group, groups);
  LVAE_REQUIRE((int64_t)qtiles * groups <= INT32_MAX, LVAE_EINVAL, "lvae_nn_l2_f32: %d query tiles x %d row groups exceed one launch", qtiles, groups);
  const size_t need = lvae_nn_l2_workspace(Q, N, k);
  LVAE_REQUIRE(workspace && workspace_bytes >= need, LVAE_EWORKSPACE, "lvae_nn_l2_f32: workspace of %zu bytes, %zu needed",
               workspace ? workspace_bytes : (size_t)0, need);
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, LVAE_EALIGN, "lvae_nn_l2_f32: workspace is not 8-byte aligned");
  LVAE_REQUIRE((reinterpret_cast<uintptr_t>(queries) & 3) == 0 && (reinterpret_cast<uintptr_t>(dist_out) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(index_out) & 3) == 0 && (reinterpret_cast<uintptr_t>(exclude) & 3) == 0 &&
                   (table_kind == LVAE_FEED_U8 || (reinterpret_cast<uintptr_t>(table) & 3) == 0),
               LVAE_EALIGN, "lvae_nn_l2_f32: a float32 or int32 buffer is not 4-byte aligned");
  unsigned long long* cand = static_cast<unsigned long long*>(workspace);
  const NnPairArgs p{queries, table, exclude, cand, N, D, Q, k, slabs, per_group, groups};
  const dim3 grid((unsigned)(qtiles * groups));
  // static LDS only, below the default limit
  int rc = table_kind == LVAE_FEED_F32
               ? launch_lds<nn_pairs_kernel<true>>("nn_l2 (pairs)", grid, dim3(256), 0, 64 * 1024, (hipStream_t)stream, p)
               : launch_lds<nn_pairs_kernel<false>>("nn_l2 (pairs)", grid, dim3(256), 0, 64 * 1024, (hipStream_t)stream, p);
  if (rc) return rc;
  const NnMergeArgs m{cand, groups, k, index_out, dist_out};
  return launch_lds<nn_merge_kernel>("nn_l2 (merge)", dim3(Q), dim3(256), 0, 64 * 1024, (hipStream_t)stream, m);
}

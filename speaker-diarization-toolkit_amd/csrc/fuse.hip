// Fusing several diarizations of a recording (fuse.py): DOVER-Lap label mapping and weighted voting on the packed frame grid
// (packed_grid.hpp).  H hypotheses per recording, each a 64-bit speaker mask per frame; groups (h, r) are h-major, spk_off [H R + 1] holds
// the prefix sums of their speaker counts.  Pairs (a, b), a < b, are numbered p = a (2 H - a - 1) / 2 + (b - a - 1); pair group q = p R + r.
//
//   fuse_masks_kernel     speakers [G][2] of one hypothesis -> mask [G] uint64.  Thread = frame.
//   fuse_cooccur_kernel   grid (frame blocks, pairs): a workgroup takes FUSE_NT consecutive packed frames of one pair and serves the recordings
//                         inside them one at a time (pg_walk): the pair's [K_a][K_b] table is summed in LDS (at most 64 x 64 int32, 16 KB),
//                         then one integer atomic add per non-zero cell; tally [q][2] = (sum max(n_a, n_b), sum min(n_a, n_b)).
//   (sdk_score_map runs between the two on the pair tables as they stand: correct [P R])
//   fuse_labels_kernel    one wave per recording: the disagreement matrix, the rank order, the weights, and the greedy label map.  The
//                         agreement table A [L][K_h] (int64, 32 KB of LDS) is built with lane = column; the arg-max of a greedy step is a wave
//                         reduction over (value, u, j), each lane bringing the best free row of its column, rescanned only when that row is taken.
//   fuse_vote_kernel      thread = frame: the weighted vote over the labels the frame's hypotheses see.  The set bits of the union are walked
//                         with a running best two (no per-label array: nothing lives in scratch); the three per-frame tallies are summed per
//                         workgroup and recording, then one integer atomic each.
//
// Integers only: stores of one value and integer adds, so every output is bit-identical run to run.  No kernel needs an ordering between
// workgroups of one launch: the launches follow each other in stream order.
#include "common.hpp"
#include "packed_grid.hpp"
#include "reduce.hpp"

namespace {

constexpr int FUSE_NT = 256;                 // frames per workgroup (fuse.FUSE_BLOCK_FRAMES)
constexpr int FUSE_MAX_HYPS = 8;             // fuse.MAX_FUSE_HYPS: at most 28 pairs

// the bits 0 .. K - 1 (K = 64: all of them; 1 << 64 is undefined)
__device__ __forceinline__ unsigned long long fuse_valid(int K) { return K >= 64 ? ~0ull : ((1ull << K) - 1ull); }

// pair p of H hypotheses -> (a, b), a < b
__host__ __device__ __forceinline__ void fuse_pair(int p, int H, int& a, int& b) {
  a = 0;
  while (p >= H - 1 - a) { p -= H - 1 - a; ++a; }
  b = a + 1 + p;
}
__host__ __device__ __forceinline__ int fuse_pair_index(int a, int b, int H) { return a * (2 * H - a - 1) / 2 + (b - a - 1); }

__global__ __launch_bounds__(FUSE_NT) void fuse_masks_kernel(const int32_t* __restrict__ speakers, const int32_t* __restrict__ frame_off,
                                                             const int32_t* __restrict__ spk_off, int R, int G,
                                                             unsigned long long* __restrict__ mask) {
  const int64_t gw = (int64_t)blockIdx.x * FUSE_NT + threadIdx.x;
  if (gw >= G) return;
  const int g = (int)gw;
  const int r = pg_find_group(frame_off, R, g);
  const int K = pg_speakers(spk_off, r);
  const int2 h = reinterpret_cast<const int2*>(speakers)[g];
  unsigned long long m = 0;
  if (h.x >= 0 && h.x < K) m |= 1ull << h.x;
  if (h.y >= 0 && h.y < K) m |= 1ull << h.y;
  mask[g] = m;
}

__global__ __launch_bounds__(FUSE_NT) void fuse_cooccur_kernel(const unsigned long long* __restrict__ mask, const int32_t* __restrict__ frame_off,
                                                               const int32_t* __restrict__ spk_off, const int64_t* __restrict__ co_off, int H,
                                                               int R, int G, int32_t* __restrict__ co, unsigned long long* __restrict__ tally) {
  __shared__ int32_t tab[PG_MAX_SPK * PG_MAX_SPK];
  __shared__ int32_t tal[2];
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  int ha, hb;
  fuse_pair(p, H, ha, hb);
  const unsigned long long* __restrict__ ma_all = mask + (int64_t)ha * G;
  const unsigned long long* __restrict__ mb_all = mask + (int64_t)hb * G;
  const int f0 = blockIdx.x * FUSE_NT;
  pg_walk(frame_off, R, f0, min(f0 + FUSE_NT, G), [&](int r, int a, int b) {
    const int Ka = pg_speakers(spk_off, ha * R + r), Kb = pg_speakers(spk_off, hb * R + r);
    const int64_t q = (int64_t)p * R + r;
    pg_co_clear<2, FUSE_NT>(tab, tal, Ka * Kb);
    int n_max = 0, n_min = 0;
    const unsigned long long va = fuse_valid(Ka), vb = fuse_valid(Kb);
    for (int g = a + tid; g < b; g += FUSE_NT) {
      unsigned long long ma = ma_all[g] & va;
      const unsigned long long mb = mb_all[g] & vb;
      const int na = __popcll(ma), nb = __popcll(mb);
      n_max += max(na, nb);
      n_min += min(na, nb);
      while (ma) {
        const int i = __ffsll((long long)ma) - 1;
        ma &= ma - 1;
        unsigned long long m = mb;
        while (m) {
          const int j = __ffsll((long long)m) - 1;
          m &= m - 1;
          atomicAdd(&tab[i * Kb + j], 1);
        }
      }
    }
    pg_co_flush<2, FUSE_NT>(tab, tal, {n_max, n_min}, Ka * Kb, co + co_off[q], tally + 2 * q);
  });
}

struct FuseKey { long long v; int u, j; };
// the largest v; ties to the least u, then the least j
__device__ __forceinline__ FuseKey fuse_wave_argmax(long long v, int u, int j) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = __shfl_xor(v, o, 64);
    const int ou = __shfl_xor(u, o, 64), oj = __shfl_xor(j, o, 64);
    if (ov > v || (ov == v && (ou < u || (ou == u && oj < j)))) { v = ov; u = ou; j = oj; }
  }
  return {v, u, j};
}

// the best free row of column j of A [64][64]: the largest A[u][j] > 0 over u < L not in `used`, the least u at equal values; none: (0, 64)
__device__ __forceinline__ void fuse_column_best(const long long* A, int j, int L, unsigned long long used, long long& bv, int& bu) {
  bv = 0;
  bu = PG_MAX_SPK;
  for (int u = 0; u < L; ++u) {
    const long long x = A[u * PG_MAX_SPK + j];
    if (!((used >> u) & 1ull) && x > bv) { bv = x; bu = u; }
  }
}

__global__ __launch_bounds__(64) void fuse_labels_kernel(const int32_t* __restrict__ co, const long long* __restrict__ tally,
                                                         const long long* __restrict__ correct, const int32_t* __restrict__ spk_off,
                                                         const int64_t* __restrict__ co_off, const int32_t* __restrict__ rank_weight,
                                                         const int32_t* __restrict__ weights, int H, int R, long long* __restrict__ dis,
                                                         int32_t* __restrict__ order, int32_t* __restrict__ weight,
                                                         int32_t* __restrict__ label_of, int32_t* __restrict__ n_labels,
                                                         int32_t* __restrict__ overflow) {
  __shared__ long long A[PG_MAX_SPK * PG_MAX_SPK];
  __shared__ long long s_dis[FUSE_MAX_HYPS * FUSE_MAX_HYPS];
  __shared__ long long s_D[FUSE_MAX_HYPS];
  __shared__ int32_t s_order[FUSE_MAX_HYPS];
  __shared__ int32_t s_label[FUSE_MAX_HYPS * PG_MAX_SPK];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int P = H * (H - 1) / 2;

  // 2 disagreement and rank
  if (lane < FUSE_MAX_HYPS * FUSE_MAX_HYPS) s_dis[lane] = 0;
  __syncthreads();
  if (lane < P) {
    int a, b;
    fuse_pair(lane, H, a, b);
    const int64_t q = (int64_t)lane * R + r;
    const long long d = tally[2 * q] - correct[q];
    s_dis[a * FUSE_MAX_HYPS + b] = d;
    s_dis[b * FUSE_MAX_HYPS + a] = d;
  }
  __syncthreads();
  if (lane < H) {
    long long D = 0;
    for (int b = 0; b < H; ++b) D += s_dis[lane * FUSE_MAX_HYPS + b];
    s_D[lane] = D;
  }
  if (lane < H * H) dis[((int64_t)r * H + lane / H) * H + lane % H] = s_dis[(lane / H) * FUSE_MAX_HYPS + lane % H];
  __syncthreads();
  if (lane < H) {
    const long long D = s_D[lane];
    int rank = 0;
    for (int b = 0; b < H; ++b) {
      const long long Db = s_D[b];
      rank += (Db < D || (Db == D && b < lane)) ? 1 : 0;
    }
    s_order[rank] = lane;
    order[(int64_t)r * H + rank] = lane;
    weight[(int64_t)r * H + lane] = weights ? weights[lane] : rank_weight[rank];
  }
  for (int c = lane; c < FUSE_MAX_HYPS * PG_MAX_SPK; c += 64) s_label[c] = -1;
  __syncthreads();

  // 3 labels
  const int anchor = s_order[0];
  int L = pg_speakers(spk_off, anchor * R + r);
  int over = 0;
  if (lane < L) {
    s_label[anchor * PG_MAX_SPK + lane] = lane;
    label_of[spk_off[anchor * R + r] + lane] = lane;
  }
  __syncthreads();
  for (int k = 1; k < H; ++k) {
    const int h = s_order[k];
    const int Kh = pg_speakers(spk_off, h * R + r);
    for (int u = 0; u < L; ++u) A[u * PG_MAX_SPK + lane] = 0;
    for (int kk = 0; kk < k; ++kk) {                            // the earlier hypotheses: lane = column j owns A[.][j]
      const int hp = s_order[kk];
      const int Kp = pg_speakers(spk_off, hp * R + r);
      const bool flip = hp > h;                                 // the pair's table is [K_h][K_hp]: read transposed
      const int p = flip ? fuse_pair_index(h, hp, H) : fuse_pair_index(hp, h, H);
      const int32_t* __restrict__ src = co + co_off[(int64_t)p * R + r];
      for (int i = 0; i < Kp; ++i) {
        const int u = s_label[hp * PG_MAX_SPK + i];
        if (u >= 0 && lane < Kh) A[u * PG_MAX_SPK + lane] += flip ? src[lane * Kp + i] : src[i * Kh + lane];
      }
    }
    // (every lane reads and writes its own column only: no barrier is needed before the greedy steps)
    unsigned long long used = 0;
    bool mapped = lane >= Kh;                                   // lanes past K_h never enter
    int mine = -1;
    long long bv;
    int bu;
    fuse_column_best(A, lane, L, used, bv, bu);
    for (;;) {
      const FuseKey best = fuse_wave_argmax(mapped ? 0 : bv, mapped ? PG_MAX_SPK : bu, lane);
      if (best.v <= 0) break;                                   // uniform: every lane holds the same key
      used |= 1ull << best.u;
      if (lane == best.j) { mapped = true; mine = best.u; }
      else if (!mapped && bu == best.u) fuse_column_best(A, lane, L, used, bv, bu);
    }
    const bool fresh = !mapped;                                 // the unmapped speakers, in ascending j
    const unsigned long long bal = __ballot(fresh);
    if (fresh) {
      const int at = L + __popcll(bal & ((1ull << lane) - 1ull));
      mine = at < PG_MAX_SPK ? at : -1;
    }
    const int n_new = __popcll(bal);
    over += max(0, L + n_new - PG_MAX_SPK);
    L = min(PG_MAX_SPK, L + n_new);
    if (lane < Kh) {
      s_label[h * PG_MAX_SPK + lane] = mine;
      label_of[spk_off[h * R + r] + lane] = mine;
    }
    __syncthreads();
  }
  if (lane == 0) {
    n_labels[r] = L;
    overflow[r] = over;
  }
}

__global__ __launch_bounds__(FUSE_NT) void fuse_tally_init_kernel(const int32_t* __restrict__ overflow, int R, long long* __restrict__ tallies) {
  const int r = blockIdx.x * FUSE_NT + threadIdx.x;
  if (r >= R) return;
  tallies[4 * (int64_t)r] = 0;
  tallies[4 * (int64_t)r + 1] = 0;
  tallies[4 * (int64_t)r + 2] = 0;
  tallies[4 * (int64_t)r + 3] = overflow[r];
}

__global__ __launch_bounds__(FUSE_NT) void fuse_vote_kernel(const unsigned long long* __restrict__ mask, const int32_t* __restrict__ frame_off,
                                                            const int32_t* __restrict__ spk_off, const int32_t* __restrict__ label_of,
                                                            const int32_t* __restrict__ weight, int H, int R, int G, int cap,
                                                            int32_t* __restrict__ speakers, unsigned long long* __restrict__ tallies) {
  __shared__ int32_t tal[3];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * FUSE_NT;
  pg_walk(frame_off, R, f0, min(f0 + FUSE_NT, G), [&](int r, int a, int b) {
    if (tid < 3) tal[tid] = 0;
    __syncthreads();
    const int g = f0 + tid;
    int speech = 0, overlap = 0, unanimous = 0;
    if (g >= a && g < b) {
      unsigned long long seen[FUSE_MAX_HYPS];
      int w[FUSE_MAX_HYPS];
      unsigned long long all = 0;
      long long wc = 0, W = 0;
      bool same = true;
#pragma unroll
      for (int h = 0; h < FUSE_MAX_HYPS; ++h) {                 // unrolled: seen and w stay in registers
        seen[h] = 0;
        w[h] = 0;
        if (h < H) {
          const int K = pg_speakers(spk_off, h * R + r);
          const int32_t* __restrict__ lab = label_of + spk_off[h * R + r];
          unsigned long long m = mask[(int64_t)h * G + g] & fuse_valid(K);
          w[h] = weight[(int64_t)r * H + h];
          wc += (long long)w[h] * __popcll(m);
          W += w[h];
          unsigned long long s = 0;
          while (m) {
            const int i = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int u = lab[i];
            if (u >= 0 && u < PG_MAX_SPK) s |= 1ull << u;
          }
          seen[h] = s;
          all |= s;
          same = same && s == seen[0];
        }
      }
      const int n = (int)min((long long)cap, (2 * wc + W) / (2 * W));
      int u0 = -1, u1 = -1;
      long long v0 = 0, v1 = 0;                                 // the best two by (v descending, u ascending): u ascends, so `>` keeps the lower
      while (all) {
        const int u = __ffsll((long long)all) - 1;
        all &= all - 1;
        long long v = 0;
#pragma unroll
        for (int h = 0; h < FUSE_MAX_HYPS; ++h) v += ((seen[h] >> u) & 1ull) ? w[h] : 0;
        if (v > v0) { v1 = v0; u1 = u0; v0 = v; u0 = u; }
        else if (v > v1) { v1 = v; u1 = u; }
      }
      const int o0 = n >= 1 ? u0 : -1, o1 = n >= 2 ? u1 : -1;
      reinterpret_cast<int2*>(speakers)[g] = make_int2(o0, o1);
      speech = o0 >= 0;
      overlap = o1 >= 0;
      unanimous = same;
    }
    const int s0 = wave_sum(speech), s1 = wave_sum(overlap), s2 = wave_sum(unanimous);
    if ((tid & 63) == 0) {
      if (s0) atomicAdd(&tal[0], s0);
      if (s1) atomicAdd(&tal[1], s1);
      if (s2) atomicAdd(&tal[2], s2);
    }
    __syncthreads();
    if (tid < 3 && tal[tid]) atomicAdd(tallies + 4 * (int64_t)r + tid, (unsigned long long)tal[tid]);
    __syncthreads();
  });
}

}  // namespace

#define FUSE_REQUIRE_SHAPE(who, H, R, G, max_spk)                                                                                            \
  SDK_REQUIRE((H) >= 2 && (H) <= FUSE_MAX_HYPS, who ": H=%d hypotheses (2 .. %d)", (H), FUSE_MAX_HYPS);                                    \
  SDK_REQUIRE((R) >= 1 && (R) < (1 << 20) && (G) >= 0 && (G) < (1ll << 30), who ": R=%d G=%lld (R 1 .. 2^20 - 1, fewer than 2^30 frames)", \
              (R), (long long)(G));                                                                                                          \
  SDK_REQUIRE((max_spk) >= 0 && (max_spk) <= PG_MAX_SPK, who ": %d speakers in a hypothesis (at most %d)", (max_spk), PG_MAX_SPK)

extern "C" int sdk_fuse_masks(sdk_ctx* ctx, const int32_t* speakers, const int32_t* frame_off, const int32_t* spk_off, int R, int64_t G, int max_spk,
                              uint64_t* mask, void* stream) {
  SDK_REQUIRE(ctx, "sdk_fuse_masks: null context");
  FUSE_REQUIRE_SHAPE("sdk_fuse_masks", 2, R, G, max_spk);
  if (G == 0) return 0;
  SDK_REQUIRE(speakers && frame_off && spk_off && mask, "sdk_fuse_masks: null argument");
  SDK_REQUIRE(((uintptr_t)speakers & 7) == 0, "sdk_fuse_masks: speakers=%p must be 8-byte aligned", (const void*)speakers);
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 16.0 * G);
  hipLaunchKernelGGL(fuse_masks_kernel, pg_grid(G, FUSE_NT), dim3(FUSE_NT), 0, (hipStream_t)stream, speakers, frame_off, spk_off, R, (int)G,
                     (unsigned long long*)mask);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_fuse_cooccur(sdk_ctx* ctx, const uint64_t* mask, const int32_t* frame_off, const int32_t* spk_off, const int64_t* co_off, int H,
                                int R, int64_t G, int max_spk, int64_t co_total, int32_t* co, int64_t* tally, void* stream) {
  SDK_REQUIRE(ctx, "sdk_fuse_cooccur: null context");
  FUSE_REQUIRE_SHAPE("sdk_fuse_cooccur", H, R, G, max_spk);
  SDK_REQUIRE(co_total >= 0, "sdk_fuse_cooccur: co_total=%lld", (long long)co_total);
  SDK_REQUIRE(tally && (co_total == 0 || co), "sdk_fuse_cooccur: null argument (co=%p tally=%p)", (void*)co, (void*)tally);
  const int P = H * (H - 1) / 2;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, 16.0 * G * P + 4.0 * co_total);
  SDK_HIP_OK(hipMemsetAsync(tally, 0, (size_t)P * R * 2 * 8, s));
  if (co_total) SDK_HIP_OK(hipMemsetAsync(co, 0, (size_t)co_total * 4, s));
  if (G == 0) return 0;
  SDK_REQUIRE(mask && frame_off && spk_off && co_off, "sdk_fuse_cooccur: null argument");
  dim3 grid = pg_grid(G, FUSE_NT);
  grid.y = P;
  hipLaunchKernelGGL(fuse_cooccur_kernel, grid, dim3(FUSE_NT), 0, s, (const unsigned long long*)mask, frame_off, spk_off, co_off, H, R, (int)G, co,
                     (unsigned long long*)tally);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_fuse_labels(sdk_ctx* ctx, const int32_t* co, const int64_t* tally, const int64_t* correct, const int32_t* spk_off,
                               const int64_t* co_off, const int32_t* rank_weight, const int32_t* weights, int H, int R, int max_spk, int64_t* dis,
                               int32_t* order, int32_t* weight, int32_t* label_of, int32_t* n_labels, int32_t* overflow, void* stream) {
  SDK_REQUIRE(ctx, "sdk_fuse_labels: null context");
  FUSE_REQUIRE_SHAPE("sdk_fuse_labels", H, R, 0, max_spk);
  SDK_REQUIRE(tally && correct && spk_off && co_off && (rank_weight || weights) && dis && order && weight && n_labels && overflow &&
                  (max_spk == 0 || (co && label_of)),
              "sdk_fuse_labels: null argument");
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (double)R * H * (4.0 * H * max_spk * max_spk + 8.0 * H + 4.0 * max_spk));
  hipLaunchKernelGGL(fuse_labels_kernel, dim3(R), dim3(64), 0, (hipStream_t)stream, co, (const long long*)tally, (const long long*)correct, spk_off, co_off,
                     rank_weight, weights, H, R, (long long*)dis, order, weight, label_of, n_labels, overflow);
  SDK_LAUNCH_CHECK();
  return 0;
}

extern "C" int sdk_fuse_vote(sdk_ctx* ctx, const uint64_t* mask, const int32_t* frame_off, const int32_t* spk_off, const int32_t* label_of,
                             const int32_t* weight, const int32_t* overflow, int H, int R, int64_t G, int max_spk, int cap, int32_t* speakers,
                             int64_t* tallies, void* stream) {
  SDK_REQUIRE(ctx, "sdk_fuse_vote: null context");
  FUSE_REQUIRE_SHAPE("sdk_fuse_vote", H, R, G, max_spk);
  SDK_REQUIRE(cap == 1 || cap == 2, "sdk_fuse_vote: cap=%d (1 or 2 speakers per frame)", cap);
  SDK_REQUIRE(overflow && tallies, "sdk_fuse_vote: null argument (overflow=%p tallies=%p)", (const void*)overflow, (void*)tallies);
  if (G > 0) {
    SDK_REQUIRE(mask && frame_off && spk_off && weight && speakers && (max_spk == 0 || label_of), "sdk_fuse_vote: null argument");
    SDK_REQUIRE(((uintptr_t)speakers & 7) == 0, "sdk_fuse_vote: speakers=%p must be 8-byte aligned", (void*)speakers);
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(ctx, stream, SDK_K_COPY, 0.0, (8.0 * H + 8.0) * G + 32.0 * R);
  hipLaunchKernelGGL(fuse_tally_init_kernel, pg_grid(R, FUSE_NT), dim3(FUSE_NT), 0, s, overflow, R, (long long*)tallies);
  if (G > 0)
    hipLaunchKernelGGL(fuse_vote_kernel, pg_grid(G, FUSE_NT), dim3(FUSE_NT), 0, s, (const unsigned long long*)mask, frame_off, spk_off, label_of, weight, H, R,
                       (int)G, cap, speakers, (unsigned long long*)tallies);
  SDK_LAUNCH_CHECK();
  return 0;
}

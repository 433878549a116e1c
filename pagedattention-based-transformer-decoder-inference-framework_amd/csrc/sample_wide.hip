// Token choice over a vocabulary row that no workgroup can hold: 65,536 < V <=
// 2^20 (and any smaller V through the *_wide entries).  One workgroup of
// kSampleThreads per row, as csrc/sample.hip and csrc/logprobs.hip have it, but
// the row stays in memory (the fp32 logits the LM head just wrote, L2 /
// Infinity-Cache resident) and is STREAMED in a few coalesced passes of 16-byte
// loads in token order; only small state lives in LDS (~45 KB static).
//
// sample_wide_kernel -- the semantics stated at the top of csrc/sample.hip:
//   pass 1  running max and sum(exp) per thread in one pass (the sum rescaled
//           when the max rises), the threads' (m, s) combined in a fixed order.
//           A greedy row ends here with its first maximum.
//   pass 2  histogram radix select.  p = exp(x / T - m) / (s + 1e-6) has a
//           non-negative fp32 bit pattern <= 0x3F800000; its leading 11 bits
//           index 2,048 LDS bins that take a COUNT (top-k) and a MASS (top-p)
//           per bin in the one pass.  Mass is fixed point, p * 2^40 as uint64,
//           added with integer LDS atomics: the sums are exact and independent
//           of the order the atomics land in, so thresholds and draw are the
//           same bits on every launch and graph replay.  V <= 2^20 keeps every
//           sum below 2^60.  A suffix scan over the bins names the bin that
//           holds the k-th largest pattern and the bin where the mass ranked
//           above reaches top_p.
//   pass 3  refinement of the other 20 bits, two more digit histograms (11 and
//           9 bits) per threshold.  The tokens of a threshold bin are compacted
//           into an LDS candidate list (kCand patterns) in one row pass and the
//           digit histograms run over the list; a bin that overflows its list
//           (a row of equal logits puts all V tokens into one) takes its two
//           histograms from the row instead.  Every loop is bounded by V and
//           the digit count: nothing waits on memory.
//   pass 4  the draw.  Kept mass per 2,048-token tile (one wave per tile, token
//           order), a block scan of the tile sums finds the first tile whose
//           inclusive sum exceeds target = floor(u * Z), and wave 0 rescans that
//           one tile to the token.  Integer sums tile [0, Z) exactly: no claim
//           gaps to repair, unlike the fp32 scan of sample_rows_kernel.
// A row without top-k (top_k 0 or >= V) takes no count select, one without
// top-p (top_p >= 1) accumulates no mass; with neither, passes 2 and 3 vanish.
//
// logprob_wide_kernel -- logprob_rows_kernel's contract in ONE pass: each thread
// keeps its own sorted top-n (logit descending, id ascending) in registers
// beside the running (m, s); the 512 lists merge through LDS, wave then block,
// under the same order.  Nothing is masked and no rounded value is ranked.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "row_ops.hpp"
#include "row_vals.hpp"
#include "sample_args.hpp"

namespace llm {
namespace {

constexpr int kBins = 2048;      // leading digit: pattern bits 30..20
constexpr int kCand = 2048;      // candidate list capacity per threshold
constexpr int kNoTok = 0x7fffffff;
constexpr float kFix = 1099511627776.f;  // 2^40

// Vec j of a row covers the four tokens 4j - mis .. 4j - mis + 3, where mis is
// the row's offset (in floats) from 16-byte alignment: every vec but the first
// and the last is one aligned 16-byte load, and those two are scalar loads of
// their tokens inside [0, V) only.  Positions outside the row read as -inf.
struct RowStream {
  const float* lg;
  int V, mis, nvec;
  __device__ RowStream(const float* p, int v)
      : lg(p), V(v), mis((int)(((uintptr_t)p >> 2) & 3)), nvec((mis + v + 3) >> 2) {}
  __device__ __forceinline__ bool valid(int e) const { return (unsigned)e < (unsigned)V; }
  __device__ __forceinline__ int load(int j, float (&x)[4]) const {
    const int e0 = 4 * j - mis;
    if (e0 >= 0 && e0 + 4 <= V) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lg + e0);
      x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = valid(e0 + c) ? lg[e0 + c] : -INFINITY;
    }
    return e0;
  }
  // f(token, logit) over the row's tokens, thread t taking vecs t, t + 512, ..
  template <typename F>
  __device__ __forceinline__ void each(F f) const {
    for (int j = threadIdx.x; j < nvec; j += kSampleThreads) {
      float x[4];
      const int e0 = load(j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (valid(e0 + c)) f(e0 + c, x[c]);
    }
  }
};

// Running (max, sum exp(x - max)) over one vec; -inf entries add nothing.
__device__ __forceinline__ void online_add(const float (&x)[4], float& m, float& s) {
  const float vm = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
  if (vm > m) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (x[c] > m) {
        s = s * expf(m - x[c]) + 1.f;
        m = x[c];
      } else if (m > -INFINITY) {
        s += expf(x[c] - m);
      }
    }
  } else if (m > -INFINITY) {
    s += (expf(x[0] - m) + expf(x[1] - m)) + (expf(x[2] - m) + expf(x[3] - m));
  }
}

// The probability every pass recomputes from the logit: one expression, so the
// same bits each time.  NaN counts as 0.
__device__ __forceinline__ float prob_of(float x, float T, float m, float inv) {
  const float p = expf(x / T - m) * inv;
  return p > 0.f ? fminf(p, 1.f) : 0.f;
}
__device__ __forceinline__ uint64_t fix_of(float p) { return (uint64_t)(p * kFix); }

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += shfl_u64(v, lane_id() ^ off);
  return v;
}
__device__ __forceinline__ uint64_t wave_scan_u64(uint64_t v) {  // inclusive, lane order
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t t = shfl_u64(v, max(lane_id() - off, 0));
    if (lane_id() >= off) v += t;
  }
  return v;
}

// Inclusive scan over the workgroup in thread order; sh[kSampleThreads - 1]
// holds the total afterwards.
__device__ __forceinline__ uint64_t block_scan(uint64_t v, uint64_t* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < kSampleThreads; off <<= 1) {
    const uint64_t t = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  return sh[threadIdx.x];
}

// State of the two radix selects, one per threshold.
struct Select {
  uint32_t pref_k;  // resolved leading bits of the k-th largest pattern
  uint32_t rem_k;   // its rank among the patterns that share them (>= 1)
  uint32_t cnt_k;   // tokens in the bin just chosen
  uint32_t pref_p;  // resolved leading bits of the smallest kept pattern
  uint32_t cnt_p;
  uint64_t acc_p;   // mass of the patterns above those that share pref_p
  uint32_t n_k, n_p;  // candidate list lengths
  int tile;
  uint64_t base;
};

// One digit of both selects from the filled histograms (thread t owns bins
// 4t .. 4t + 3).  top-k: the bin b with  above(b) < rem_k <= above(b) + cnt[b].
// top-p: the lowest bin b whose mass above, acc_p + above(b), is < P -- the
// smallest kept pattern lies in it (a token is kept iff the mass strictly above
// it is < P).  Exactly one thread writes each.
__device__ __forceinline__ void select_digit(int shift, bool do_k, bool do_p, uint64_t P,
                                             const uint32_t* cnt, const uint64_t* mass,
                                             uint64_t* scan, Select* sel) {
  const int b0 = 4 * threadIdx.x;
  if (do_k) {
    const uint32_t k = sel->rem_k;
    uint32_t c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = cnt[b0 + i];
    const uint64_t incl = block_scan((uint64_t)c[0] + c[1] + c[2] + c[3], scan);
    uint32_t above = (uint32_t)(scan[kSampleThreads - 1] - incl);
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if (above < k && above + c[i] >= k) {
        sel->pref_k |= (uint32_t)(b0 + i) << shift;
        sel->rem_k = k - above;
        sel->cnt_k = c[i];
      }
      above += c[i];
    }
  }
  if (do_p) {
    const uint64_t acc = sel->acc_p;
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = mass[b0 + i];
    const uint64_t incl = block_scan((w[0] + w[1]) + (w[2] + w[3]), scan);
    uint64_t above = acc + (scan[kSampleThreads - 1] - incl);
#pragma unroll
    for (int i = 3; i >= 0; --i) {
      if (above < P && (b0 + i == 0 || above + w[i] >= P)) {
        sel->pref_p |= (uint32_t)(b0 + i) << shift;
        sel->acc_p = above;
        sel->cnt_p = cnt[b0 + i];
      }
      above += w[i];
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void write_token(const SampleArgs& a, int r, int tok) {
  a.out[r] = tok;
  if (a.out2) a.out2[(size_t)r * a.out2_stride] = tok;
}

__global__ __launch_bounds__(kSampleThreads) void sample_wide_kernel(SampleArgs a) {
  __shared__ uint32_t cnt[kBins];
  __shared__ uint64_t mass[kBins];  // pass 4: the tile sums
  __shared__ uint32_t list_k[kCand], list_p[kCand];
  __shared__ uint64_t scan[kSampleThreads];
  __shared__ float shf[16];
  __shared__ int shi[16];
  __shared__ Select sel;
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const RowStream row(a.logits + (size_t)r * a.V, a.V);
  const float T = a.temperature_v ? a.temperature_v[r] : a.temperature;
  const int top_k = a.top_k_v ? a.top_k_v[r] : a.top_k;
  const float top_p = a.top_p_v ? a.top_p_v[r] : a.top_p;

  // ---- pass 1 ---------------------------------------------------------------
  if (T <= 0.f || top_k == 1) {  // greedy: the first maximum of the raw logits
    float best = -INFINITY;
    int bi = kNoTok;
    row.each([&](int t, float x) {  // (a thread meets its tokens in ascending order)
      if (x > best) { best = x; bi = t; }
    });
    const float m = block_reduce(best, shf, [](float x, float y) { return fmaxf(x, y); });
    int cand = best == m ? bi : kNoTok;
    cand = block_reduce(cand, shi, [](int x, int y) { return min(x, y); });
    if (tid == 0) write_token(a, r, cand == kNoTok ? 0 : cand);
    return;
  }
  float ml = -INFINITY, sl = 0.f;
  for (int j = tid; j < row.nvec; j += kSampleThreads) {
    float x[4];
    row.load(j, x);
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = x[c] / T;
    online_add(x, ml, sl);
  }
  const float m = block_reduce(ml, shf, [](float x, float y) { return fmaxf(x, y); });
  if (!(fabsf(m) < INFINITY)) {  // no finite logit (or NaN): no kept mass
    if (tid == 0) write_token(a, r, 0);
    return;
  }
  sl = ml > -INFINITY ? sl * expf(ml - m) : 0.f;
  const float s = block_reduce(sl, shf, [](float x, float y) { return x + y; });
  const float inv = 1.0f / (s + 1e-6f);

  // ---- passes 2 and 3: keep patterns >= thr ----------------------------------
  const bool need_k = top_k > 1 && top_k < a.V;
  const bool need_p = top_p < 1.0f;
  // mass >= top_p * 2^40  <=>  mass >= P  (the masses are integers)
  const uint64_t P = top_p > 0.f ? (uint64_t)ceil((double)top_p * (double)kFix) : 1;
  uint32_t thr = 0;
  if (need_k || need_p) {
    for (int i = tid; i < kBins; i += kSampleThreads) { cnt[i] = 0; mass[i] = 0; }
    if (tid == 0) {
      sel.pref_k = 0; sel.rem_k = (uint32_t)top_k; sel.cnt_k = 0;
      sel.pref_p = 0; sel.cnt_p = 0; sel.acc_p = 0;
      sel.n_k = 0; sel.n_p = 0;
    }
    __syncthreads();
    row.each([&](int, float x) {
      const float p = prob_of(x, T, m, inv);
      const uint32_t bin = __float_as_uint(p) >> 20;
      atomicAdd(&cnt[bin], 1u);
      if (need_p) atomicAdd((unsigned long long*)&mass[bin], (unsigned long long)fix_of(p));
    });
    __syncthreads();
    select_digit(20, need_k, need_p, P, cnt, mass, scan, &sel);
    const bool lst_k = need_k && sel.cnt_k <= (uint32_t)kCand;
    const bool lst_p = need_p && sel.cnt_p <= (uint32_t)kCand;
    const uint32_t bin_k = sel.pref_k >> 20, bin_p = sel.pref_p >> 20;
    if (lst_k || lst_p) {  // compact the threshold bins' patterns
      row.each([&](int, float x) {
        const uint32_t bits = __float_as_uint(prob_of(x, T, m, inv));
        if (lst_k && (bits >> 20) == bin_k) {
          const uint32_t i = atomicAdd(&sel.n_k, 1u);
          if (i < (uint32_t)kCand) list_k[i] = bits;
        }
        if (lst_p && (bits >> 20) == bin_p) {
          const uint32_t i = atomicAdd(&sel.n_p, 1u);
          if (i < (uint32_t)kCand) list_p[i] = bits;
        }
      });
    }
    __syncthreads();
    const int n_k = min(sel.n_k, (uint32_t)kCand), n_p = min(sel.n_p, (uint32_t)kCand);
    const bool row_k = need_k && !lst_k, row_p = need_p && !lst_p;
#pragma unroll 1
    for (int level = 1; level <= 2; ++level) {
      const int prev = level == 1 ? 20 : 9, shift = level == 1 ? 9 : 0;
      const uint32_t dmask = level == 1 ? 0x7FFu : 0x1FFu;
      for (int i = tid; i < kBins; i += kSampleThreads) { cnt[i] = 0; mass[i] = 0; }
      __syncthreads();
      const uint32_t pk = sel.pref_k >> prev, pp = sel.pref_p >> prev;
      auto add_k = [&](uint32_t bits) {
        if ((bits >> prev) == pk) atomicAdd(&cnt[(bits >> shift) & dmask], 1u);
      };
      auto add_p = [&](uint32_t bits) {
        if ((bits >> prev) == pp)
          atomicAdd((unsigned long long*)&mass[(bits >> shift) & dmask],
                    (unsigned long long)fix_of(__uint_as_float(bits)));
      };
      if (lst_k) for (int i = tid; i < n_k; i += kSampleThreads) add_k(list_k[i]);
      if (lst_p) for (int i = tid; i < n_p; i += kSampleThreads) add_p(list_p[i]);
      if (row_k || row_p) {  // an overflowed bin: this digit from the row
        row.each([&](int, float x) {
          const uint32_t bits = __float_as_uint(prob_of(x, T, m, inv));
          if (row_k) add_k(bits);
          if (row_p) add_p(bits);
        });
      }
      __syncthreads();
      select_digit(shift, need_k, need_p, P, cnt, mass, scan, &sel);
    }
    thr = max(need_k ? sel.pref_k : 0u, need_p ? sel.pref_p : 0u);
  }

  // ---- pass 4: the draw --------------------------------------------------------
  uint64_t* tile_sum = mass;  // [2 * kSampleThreads] >= the row's tiles, in pairs
  __syncthreads();
  for (int i = tid; i < 2 * kSampleThreads; i += kSampleThreads) tile_sum[i] = 0;
  __syncthreads();
  const int wave = wave_id_uniform(), lane = lane_id();
  const int ntile = (row.nvec + kSampleThreads - 1) / kSampleThreads;  // <= 513
  auto kept = [&](int e, float x) -> uint64_t {
    if (!row.valid(e)) return 0;
    const float p = prob_of(x, T, m, inv);
    return __float_as_uint(p) >= thr ? fix_of(p) : 0;
  };
  for (int t = wave; t < ntile; t += kSampleThreads / 64) {
    uint64_t acc = 0;
#pragma unroll 2
    for (int i = 0; i < 8; ++i) {
      const int j = t * kSampleThreads + i * 64 + lane;
      if (j < row.nvec) {
        float x[4];
        const int e0 = row.load(j, x);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc += kept(e0 + c, x[c]);
      }
    }
    acc = wave_sum_u64(acc);
    if (lane == 0) tile_sum[t] = acc;
  }
  __syncthreads();
  const uint64_t t0 = tile_sum[2 * tid], t1 = tile_sum[2 * tid + 1];
  const uint64_t incl = block_scan(t0 + t1, scan);
  const uint64_t Z = scan[kSampleThreads - 1];
  if (Z == 0) {  // every kept probability is below 2^-40
    if (tid == 0) write_token(a, r, 0);
    return;
  }
  const int ctr = a.counter ? a.counter[r] : a.counter0;
  const float u = a.seed_v ? sample_uniform(a.seed_v[r], 0, ctr)
                           : sample_uniform(a.seed, a.row0 + r, ctr);
  const uint64_t ui = (uint64_t)(u * 16777216.0f);  // the draw's 24 bits
  // floor(u * Z) without overflow: Z < 2^60
  const uint64_t target = ui * (Z >> 24) + ((ui * (Z & 0xFFFFFFull)) >> 24);
  int own = incl > target ? tid : kNoTok;
  own = block_reduce(own, shi, [](int x, int y) { return min(x, y); });  // (< Z: one exists)
  if (tid == own) {
    const uint64_t excl = incl - (t0 + t1);
    const bool first = excl + t0 > target;
    sel.tile = 2 * tid + (first ? 0 : 1);
    sel.base = first ? excl : excl + t0;
  }
  __syncthreads();
  if (wave != 0) return;
  const int t = sel.tile;
  uint64_t base = sel.base;
  for (int i = 0; i < 8; ++i) {  // the tile's 8 wave-wide slices, token order
    const int j = t * kSampleThreads + i * 64 + lane;
    uint64_t q[4] = {0, 0, 0, 0};
    int e0 = 0;
    if (j < row.nvec) {
      float x[4];
      e0 = row.load(j, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) q[c] = kept(e0 + c, x[c]);
    }
    const uint64_t mine = (q[0] + q[1]) + (q[2] + q[3]);
    const uint64_t li = wave_scan_u64(mine);
    const uint64_t tot = shfl_u64(li, 63);
    if (base + tot > target) {
      const unsigned long long hit = __ballot(base + li > target);
      if (lane == __ffsll(hit) - 1) {
        uint64_t c = base + li - mine;
        int tok = 0;
#pragma unroll
        for (int k = 3; k >= 0; --k) {  // the first token whose inclusive sum exceeds target
          uint64_t upto = c;
          for (int z = 0; z <= k; ++z) upto += q[z];
          if (upto > target) tok = e0 + k;
        }
        write_token(a, r, tok);
      }
      return;
    }
    base += tot;
  }
}

// (logit descending, token id ascending)
__device__ __forceinline__ bool ranks_before(float a, int ai, float b, int bi) {
  return a > b || (a == b && ai < bi);
}

// N rounds of wave-wide best-of-heads over sorted lists held in LDS: lane's
// list entry q is (sv, si)[q * stride + idx]; a lane with have == false brings
// no list.  emit(round, logit, id) runs on every lane with the round's winner.
template <int N, typename F>
__device__ __forceinline__ void wave_merge(const float* sv, const int* si, int stride, int idx,
                                           bool have, F emit) {
  int ptr = have ? 0 : N;
  for (int k = 0; k < N; ++k) {
    const float hv = ptr < N ? sv[ptr * stride + idx] : -INFINITY;
    const int hi = ptr < N ? si[ptr * stride + idx] : kNoTok;
    float bv = hv;
    int bi = hi;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (ranks_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (hi == bi && hi != kNoTok) ++ptr;  // ids are unique: the winner's lane
    emit(k, bv, bi);
  }
}

template <int N>
__global__ __launch_bounds__(kSampleThreads) void logprob_wide_kernel(
    const float* __restrict__ logits, int V, const int32_t* __restrict__ chosen, int top_n,
    float* __restrict__ chosen_lp, float* __restrict__ top_lp, int32_t* __restrict__ top_id,
    float* __restrict__ stats) {
  constexpr int NN = N ? N : 1;
  constexpr int kWaves = kSampleThreads / 64;
  __shared__ float shf[16];
  __shared__ float lv[NN * kSampleThreads];  // [entry][thread]
  __shared__ int li[NN * kSampleThreads];
  __shared__ float wv[NN * kWaves];  // [entry][wave]
  __shared__ int wi[NN * kWaves];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const RowStream row(logits + (size_t)r * V, V);
  float ml = -INFINITY, sl = 0.f;
  float tv[NN];
  int ti[NN];
#pragma unroll
  for (int q = 0; q < NN; ++q) { tv[q] = -INFINITY; ti[q] = kNoTok; }
  for (int j = tid; j < row.nvec; j += kSampleThreads) {
    float x[4];
    const int e0 = row.load(j, x);
    online_add(x, ml, sl);
    if constexpr (N > 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (row.valid(e0 + c) && ranks_before(x[c], e0 + c, tv[N - 1], ti[N - 1])) {
          tv[N - 1] = x[c];
          ti[N - 1] = e0 + c;
#pragma unroll
          for (int q = N - 1; q > 0; --q) {
            if (ranks_before(tv[q], ti[q], tv[q - 1], ti[q - 1])) {
              const float fv = tv[q]; tv[q] = tv[q - 1]; tv[q - 1] = fv;
              const int fi = ti[q]; ti[q] = ti[q - 1]; ti[q - 1] = fi;
            }
          }
        }
      }
    }
  }
  const float m = block_reduce(ml, shf, [](float x, float y) { return fmaxf(x, y); });
  sl = ml > -INFINITY ? sl * expf(ml - m) : 0.f;
  const float s = block_reduce(sl, shf, [](float x, float y) { return x + y; });
  const float lse = logf(s + 1e-6f);
  if (tid == 0) {
    if (stats) { stats[2 * r] = m; stats[2 * r + 1] = lse; }
    if (chosen) {
      const int c = chosen[r];
      chosen_lp[r] = c >= 0 && c < V ? (row.lg[c] - m) - lse : 0.f;
    }
  }
  if constexpr (N > 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      lv[q * kSampleThreads + tid] = tv[q];
      li[q * kSampleThreads + tid] = ti[q];
    }
    __syncthreads();
    const int wave = wave_id_uniform(), lane = lane_id();
    wave_merge<N>(lv, li, kSampleThreads, tid, true, [&](int k, float v, int id) {
      if (lane == 0) { wv[k * kWaves + wave] = v; wi[k * kWaves + wave] = id; }
    });
    __syncthreads();
    if (wave != 0) return;
    wave_merge<N>(wv, wi, kWaves, min(lane, kWaves - 1), lane < kWaves, [&](int k, float v, int id) {
      if (lane == 0 && k < top_n) {
        top_id[(size_t)r * top_n + k] = id == kNoTok ? 0 : id;
        top_lp[(size_t)r * top_n + k] = (v - m) - lse;
      }
    });
  }
}

}  // namespace

hipError_t launch_sample_wide(const SampleArgs& a, int rows, hipStream_t st) {
  if (a.V < 1 || a.V > kWideMaxV) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_wide_kernel, dim3(rows), dim3(kSampleThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_logprob_rows_wide(const float* logits, int rows, int V, const int32_t* chosen,
                                    int top_n, float* chosen_lp, float* top_lp, int32_t* top_id,
                                    float* stats, hipStream_t st) {
  if (V < 1 || V > kWideMaxV || top_n < 0 || top_n > LLM_MAX_TOP_LOGPROBS)
    return hipErrorInvalidValue;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(kSampleThreads), 0, st, logits, V, chosen, top_n,
                       chosen_lp, top_lp, top_id, stats);
    return hipGetLastError();
  };
  // the per-thread list length: top_n rounded up, the first top_n written
  if (top_n == 0) return go(logprob_wide_kernel<0>);
  if (top_n == 1) return go(logprob_wide_kernel<1>);
  if (top_n <= 4) return go(logprob_wide_kernel<4>);
  return go(logprob_wide_kernel<8>);
}

}  // namespace llm

using namespace llm;

#define WIDE_SHAPE(name)                                                        \
  LLM_REQUIRE(rows >= 0 && V >= 1 && V <= kWideMaxV, name ": rows >= 0, 1 <= V <= 1048576")

extern "C" int sample_rows_wide(const float* logits, int rows, int V, float temperature, int top_k,
                                float top_p, uint64_t seed, int counter, int32_t* out,
                                void* stream) {
  WIDE_SHAPE("sample_rows_wide");
  LLM_REQUIRE(top_k >= 0 && top_p > 0.f && top_p <= 1.0f,
              "sample_rows_wide: top_k >= 0, 0 < top_p <= 1");
  if (rows == 0) return LLM_OK;
  LLM_REQUIRE(logits && out, "sample_rows_wide: NULL pointer");
  SampleArgs a{logits, V, temperature, top_k, top_p, seed, nullptr, counter, 0, out, nullptr, 0};
  LLM_HIP_RET(launch_sample_wide(a, rows, as_stream(stream)));
  return LLM_OK;
}

extern "C" int sample_rows_each_wide(const float* logits, int rows, int V,
                                     const float* temperature, const int32_t* top_k,
                                     const float* top_p, const uint64_t* seed,
                                     const int32_t* counter, int32_t* out, void* stream) {
  WIDE_SHAPE("sample_rows_each_wide");
  if (rows == 0) return LLM_OK;
  LLM_REQUIRE(logits && out, "sample_rows_each_wide: NULL pointer");
  SampleArgs a{logits, V, 1.0f, 0, 1.0f, 0, counter, 0, 0, out, nullptr, 0,
               temperature, top_k, top_p, seed};
  LLM_HIP_RET(launch_sample_wide(a, rows, as_stream(stream)));
  return LLM_OK;
}

extern "C" int logprob_rows_wide(const float* logits, int rows, int V, const int32_t* chosen,
                                 int top_n, float* chosen_lp, float* top_lp, int32_t* top_id,
                                 float* stats, void* stream) {
  LLM_REQUIRE(top_n >= 0 && top_n <= LLM_MAX_TOP_LOGPROBS,
              "logprob_rows_wide: top_n must be in [0, 8]");
  WIDE_SHAPE("logprob_rows_wide");
  LLM_REQUIRE(V >= top_n, "logprob_rows_wide: V < top_n");
  if (rows == 0) return LLM_OK;
  LLM_REQUIRE(logits && (!chosen || chosen_lp) && (top_n == 0 || (top_lp && top_id)),
              "logprob_rows_wide: NULL pointer");
  LLM_HIP_RET(launch_logprob_rows_wide(logits, rows, V, chosen, top_n, chosen_lp, top_lp, top_id,
                                       stats, as_stream(stream)));
  return LLM_OK;
}

// Device and host helpers of the decoder's kernels (decode.hip): map addressing, the peak sweep, the cubic and Gaussian
// weights, the std::sort replay.  Nothing here declares LDS or a kernel: the helpers are inlined into the kernels that
// call them.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "decode.h"

namespace rtpose {

struct MapView {
  const float* base;
  int cstride, choff, ws, hs, lead;
};

__device__ __forceinline__ float map_at(const MapView& m, int n, int y, int x, int c) {
  return m.base[((size_t)m.lead + (size_t)(n * m.hs + y) * m.ws + x) * m.cstride + m.choff + c];
}

constexpr int kMaxUp = 16;               // largest supported up-sampling factor
constexpr int kMaxDst = 5 * kMaxUp;      // widest up-sampled patch

// OpenCV interpolateCubic (A = -0.75f), float arithmetic, no contraction.
__device__ __forceinline__ void cubic_coeffs(float x, float* c) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

// find_peaks (paf_to_pose.py:25-38) for one (image, part): 4-neighbour maximum, > thr, peaks
// compacted in row-major order into s_px / s_py (the order defines the peak ids).  Whole block.
constexpr int kPeakBatch = 5;  // 256-pixel sweeps whose loads are in flight together (a 46 x 46 map is 8.3 sweeps: 2 batches)
__device__ __forceinline__ int find_peaks_block(const MapView& heat, int n, int part, int h, int w, float thr,
                                                int pcap, int (*s_wcount)[4], int* s_px, int* s_py, int32_t* res) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  const int npix = h * w;
  // Round 6: the CENTRE values of kPeakBatch sweeps are requested together (one global round trip per batch instead of one
  // per sweep), then the four neighbours of the few pixels above the threshold - still only of those: fetching them for every
  // pixel cost five times the loads and made the kernel slower (33 -> 43 us at batch 32) - again all sweeps' requests before
  // the first value is used; one pair of barriers per batch instead of per sweep.  The tests are the sweep-by-sweep form's.
  for (int start = 0; start < npix; start += 256 * kPeakBatch) {
    float v[kPeakBatch], vu[kPeakBatch], vd[kPeakBatch], vl[kPeakBatch], vr[kPeakBatch];
    int xs[kPeakBatch], ys[kPeakBatch];
#pragma unroll
    for (int b = 0; b < kPeakBatch; ++b) {
      const int idx = min(start + 256 * b + tid, npix - 1);
      const int y = idx / w, x = idx - y * w;
      ys[b] = y;
      xs[b] = x;
      v[b] = map_at(heat, n, y, x, part);
    }
#pragma unroll
    for (int b = 0; b < kPeakBatch; ++b) {
      vu[b] = vd[b] = vl[b] = vr[b] = 0.f;
      if (start + 256 * b + tid < npix && v[b] > thr) {  // (border neighbours: the pixel itself, ignored below)
        const int y = ys[b], x = xs[b];
        vu[b] = map_at(heat, n, max(y - 1, 0), x, part);
        vd[b] = map_at(heat, n, min(y + 1, h - 1), x, part);
        vl[b] = map_at(heat, n, y, max(x - 1, 0), part);
        vr[b] = map_at(heat, n, y, min(x + 1, w - 1), part);
      }
    }
    bool pk[kPeakBatch];
    unsigned long long mask[kPeakBatch];
#pragma unroll
    for (int b = 0; b < kPeakBatch; ++b) {
      const int x = xs[b], y = ys[b];
      bool p = start + 256 * b + tid < npix && v[b] > thr;
      if (p && y > 0) p = v[b] >= vu[b];
      if (p && y + 1 < h) p = v[b] >= vd[b];
      if (p && x > 0) p = v[b] >= vl[b];
      if (p && x + 1 < w) p = v[b] >= vr[b];
      pk[b] = p;
      mask[b] = __ballot(p);
      if (lane == 0) s_wcount[b][wave] = __popcll(mask[b]);
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < kPeakBatch; ++b) {
      int off = base;
      for (int k = 0; k < wave; ++k) off += s_wcount[b][k];
      if (pk[b]) {
        const int pos = off + __popcll(mask[b] & ((1ull << lane) - 1ull));
        if (pos < pcap) {
          s_px[pos] = xs[b];
          s_py[pos] = ys[b];
        }
      }
      base += s_wcount[b][0] + s_wcount[b][1] + s_wcount[b][2] + s_wcount[b][3];
    }
    __syncthreads();
  }
  const int count = min(base, pcap);
  if (tid == 0) {
    res[kResPartCount + part] = count;
    if (base > pcap) atomicOr(&res[kResHeader + 2], kOverflowPeaks);
  }
  return count;
}

constexpr int kGaussR = 12;  // int(truncate 4.0 * sigma 3 + 0.5)
struct GaussW {
  double w[2 * kGaussR + 1];
};

__device__ __forceinline__ int reflect_idx(int i, int n) {
  while (i < 0 || i >= n) {
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
  }
  return i;
}

// ------------------------------------------------------------------------------
// std::sort(candidates.begin(), candidates.end(), comp_candidate) (pafprocess.cpp:97, :244-246)
// as libstdc++ (GCC 11 bits/stl_algo.h - what the reference links against when built with this
// image's g++) executes it, run by ONE lane.  std::sort is not stable: when two candidates of a
// limb score exactly the same (two peaks refined to the same pixel), which one the greedy scan
// meets first is decided by the introsort's moves - median-of-3 quicksort down to 16-element
// runs under a 2 floor(log2 n) depth limit (heap sort beyond it), then one insertion pass.  The
// product is "identical to pafprocess.cpp built with g++ 11", so the rare limb with such a tie
// replays those moves on its candidate list L (entries in the reference's push order, each the
// score's bits above the pair index a * nB + b); comp(a, b) = a.score > b.score.  The list lives
// in LDS when it has at most kTieLdsCands entries (a dependent access every ~100 cycles instead
// of every ~500-2000), else in the workspace.
// ------------------------------------------------------------------------------
struct SortReplay {
  unsigned long long* L;  // entry = score bits << 32 | (a * nB + b); LDS when the list fits, else the workspace
  int* stk;               // LDS, 3 ints per pending range
  // scores are positive finite floats: their bit patterns order like their values, equal iff the floats are equal
  static __device__ __forceinline__ bool gt(unsigned long long a, unsigned long long b) {
    return (unsigned)(a >> 32) > (unsigned)(b >> 32);
  }
  __device__ __forceinline__ void swap(int i, int j) {
    const unsigned long long t = L[i];
    L[i] = L[j];
    L[j] = t;
  }
  __device__ void unguarded_linear_insert(int last) {
    const unsigned long long val = L[last];
    int next = last - 1;
    unsigned long long nv = L[next];
    while (gt(val, nv)) {
      L[last] = nv;
      last = next;
      --next;
      nv = L[next];
    }
    L[last] = val;
  }
  __device__ void insertion_sort(int first, int last) {
    if (first == last) return;
    for (int i = first + 1; i != last; ++i) {
      const unsigned long long val = L[i];
      if (gt(val, L[first])) {
        for (int k = i; k > first; --k) L[k] = L[k - 1];  // move_backward(first, i, i + 1)
        L[first] = val;
      } else {
        unguarded_linear_insert(i);
      }
    }
  }
  __device__ void push_heap(int first, int hole, int top, unsigned long long value) {
    int parent = (hole - 1) / 2;
    while (hole > top && gt(L[first + parent], value)) {
      L[first + hole] = L[first + parent];
      hole = parent;
      parent = (hole - 1) / 2;
    }
    L[first + hole] = value;
  }
  __device__ void adjust_heap(int first, int hole, int len, unsigned long long value) {
    const int top = hole;
    int child = hole;
    while (child < (len - 1) / 2) {
      child = 2 * (child + 1);
      if (gt(L[first + child], L[first + child - 1])) child--;
      L[first + hole] = L[first + child];
      hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
      child = 2 * (child + 1);
      L[first + hole] = L[first + child - 1];
      hole = child - 1;
    }
    push_heap(first, hole, top, value);
  }
  __device__ void heap_sort(int first, int last) {  // __partial_sort(first, last, last)
    const int len = last - first;
    if (len >= 2)
      for (int parent = (len - 2) / 2;; --parent) {  // __make_heap
        adjust_heap(first, parent, len, L[first + parent]);
        if (parent == 0) break;
      }
    while (last - first > 1) {  // __sort_heap
      --last;
      const unsigned long long value = L[last];
      L[last] = L[first];
      adjust_heap(first, 0, last - first, value);
    }
  }
  __device__ void move_median_to_first(int result, int a, int b, int c) {
    const unsigned long long va = L[a], vb = L[b], vc = L[c];
    if (gt(va, vb)) {
      if (gt(vb, vc)) swap(result, b);
      else if (gt(va, vc)) swap(result, c);
      else swap(result, a);
    } else if (gt(va, vc)) swap(result, a);
    else if (gt(vb, vc)) swap(result, c);
    else swap(result, b);
  }
  __device__ int unguarded_partition(int first, int last, int pivot) {
    const unsigned long long pv = L[pivot];  // (the pivot sits at `first - 1`, outside the range being swapped)
    for (;;) {
      while (gt(L[first], pv)) ++first;
      --last;
      while (gt(pv, L[last])) --last;
      if (!(first < last)) return first;
      swap(first, last);
      ++first;
    }
  }
  // __introsort_loop: the recursion on [cut, last) becomes a pending range (the ranges are
  // disjoint, so the order they are finished in does not change a single move)
  __device__ void introsort(int n, int depth_limit) {
    int sp = 0;
    stk[0] = 0;
    stk[1] = n;
    stk[2] = depth_limit;
    sp = 1;
    while (sp > 0) {
      --sp;
      int first = stk[3 * sp], last = stk[3 * sp + 1], depth = stk[3 * sp + 2];
      while (last - first > 16) {
        if (depth == 0) {
          heap_sort(first, last);
          break;
        }
        --depth;
        const int mid = first + (last - first) / 2;
        move_median_to_first(first, first + 1, mid, last - 1);
        const int cut = unguarded_partition(first + 1, last, first);
        stk[3 * sp] = cut;
        stk[3 * sp + 1] = last;
        stk[3 * sp + 2] = depth;
        ++sp;
        last = cut;
      }
    }
  }
  __device__ void sort_desc(int n) {
    if (n == 0) return;
    int lg = 0;
    while ((n >> (lg + 1)) > 0) ++lg;
    introsort(n, 2 * lg);
    if (n > 16) {
      insertion_sort(0, 16);
      for (int i = 16; i != n; ++i) unguarded_linear_insert(i);
    } else {
      insertion_sort(0, n);
    }
  }
};
constexpr int kSortStack = 3 * 64;  // pending ranges <= the depth limit 2 floor(log2 n) <= 40

constexpr int kStageWords = 5;  // per staged connection: cid1, cid2, connection score, score of peak 2, score of peak 1

static MapView to_view(const float* base, const rtpose_layout* l) {
  return MapView{base, l->cstride, l->choff, l->ws, l->hs, l->lead};
}

// scipy.ndimage._filters._gaussian_kernel1d(sigma = 3, order 0, radius 12) in float64, the sum
// taken in numpy's pairwise order (8 running partial sums, then the tail) so that the weights are
// the ones scipy correlates with, bit for bit, wherever libm's exp agrees with numpy's.
static GaussW gauss_weights() {
  GaussW g;
  const int n = 2 * kGaussR + 1;
  for (int i = -kGaussR; i <= kGaussR; ++i) g.w[i + kGaussR] = exp(-0.5 / 9.0 * (double)(i * i));
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = g.w[j];
  int i = 8;
  for (; i < n - n % 8; i += 8)
    for (int j = 0; j < 8; ++j) r[j] += g.w[i + j];
  double sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) sum += g.w[i];
  for (int k = 0; k < n; ++k) g.w[k] /= sum;
  return g;
}

}  // namespace rtpose

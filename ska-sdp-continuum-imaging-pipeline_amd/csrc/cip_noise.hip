// cip_noise.hip - the noise of an image and the island mask (cip_image_select,
// cip_image_noise, cip_auto_mask). The operators are defined in
// include/cip_noise.h.
//
// Select: a most-significant-digit radix select on order-preserving 64-bit
// keys (the sign bit flipped for positives, every bit for negatives), digits
// of 12, 13, 13, 13 and 13 bits: the first is the sign and the exponent, so
// the leading pass splits an image by binade. A pass is the histogram of the
// current digit over the samples that match the key prefix found so far; a
// one-block scan then finds the bin that holds the rank. One pass reads the
// image once (8 bytes a pixel, and 1 of the region). Once the candidates fit
// kCompactCap keys, one more read of the image packs them into a buffer and
// the remaining passes run there; while they do not fit (an all-equal image
// never shrinks) the next pass is another full one.
//
// A residual image is noise around zero, so in the first pass the 64 lanes of
// a wave fall into a handful of bins, where one LDS add per lane would
// serialise on an address. A wave adds once per distinct digit instead: one
// ballot per digit bit gives every lane the set of lanes that hold its digit,
// and the lowest lane of each set adds the set's size (wave_add): a fixed 12
// or 13 ballots whatever the values are. Every workgroup keeps its histogram
// in LDS and writes it as one row of a (grid, bins) table, which the reduce
// kernel sums by column: no global atomics, nothing to zero.
//
// Mask: one state byte per pixel (out, candidate, in). A workgroup takes a
// 32 x 64 tile and its one-pixel halo into LDS, turns candidates that touch an
// "in" pixel until the tile is stable, stores the pixels it turned and raises
// the round's flag. A byte per tile says whether anything the tile sees has
// changed since it was last stable: the seeds' tiles at first, then the eight
// neighbours of every tile that turned a pixel (written for the next round,
// so the flags are double-buffered); the other workgroups return at once. The
// host queues kMaskRoundsPerCheck rounds between two reads of the flags and
// stops when a round has changed nothing; there is no cap. Pixels only ever go from candidate to in, so a round that reads a
// neighbour's tile while it is being written sees an older or a newer state,
// and either is a state of the same monotone iteration.
#include <cmath>
#include <cstring>
#include <string>

#include "cip_host.h"
#include "cip_noise.h"

namespace cip {

namespace {

typedef unsigned long long u64;

// ------------------------------------------------------------- select ----
constexpr int kSelThreads = 1024;
constexpr int kSelMaxBlocks = 256;  // one workgroup per CU
constexpr int kSelUnroll = 4;       // 16-byte loads a thread issues together
constexpr int kSelPasses = 5;
constexpr int kSelBits[kSelPasses] = {12, 13, 13, 13, 13};
constexpr int kSelMaxBins = 1 << 13;
constexpr int64_t kCompactCap = (int64_t)1 << 16;  // keys the compacted candidates may number
static_assert(kSelBits[0] + kSelBits[1] + kSelBits[2] + kSelBits[3] + kSelBits[4] == 64, "the digits cover the key");
static_assert((1 << kSelBits[0]) % 256 == 0, "the scan gives each of 256 threads whole bins; the reduce takes 64 a workgroup");

constexpr int kModeValue = 0;      // the key of x
constexpr int kModeDeviation = 1;  // the key of |x - centre|

struct SelectState {
  u64 prefix;       // the key bits found so far
  long long rank;   // the rank among the candidates; in: the rank asked for, or < 0 for the lower median
  long long count;  // |S| (the first pass sets it)
  long long ncand;  // samples that match `prefix`
  u64 nkeys;        // keys the compaction has stored
  long long status; // 1: the rank lies outside 0 .. count - 1
};

// where a pass reads: the image (pairs from the first 16-byte aligned element,
// up to two loose elements beside them) or the compacted keys
struct SelectSource {
  const double* img;
  const uint8_t* region;
  const u64* keys;
  int64_t n;     // elements
  int64_t head;  // 1: element 0 comes before the first aligned pair
  int mode;
  double centre;
};

__device__ __forceinline__ u64 to_key(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | ((u64)1 << 63));
}

double from_key(u64 k) {
  const u64 b = (k >> 63) ? (k & ~((u64)1 << 63)) : ~k;
  double x;
  std::memcpy(&x, &b, sizeof x);
  return x;
}

// the key of element e's value x, if e is a sample
__device__ __forceinline__ bool sample_key(const SelectSource& src, double x, int64_t e, u64* key) {
  const u64 b = (u64)__double_as_longlong(x);
  if (((b >> 52) & 0x7ffu) == 0x7ffu) return false;  // NaN, +-inf
  if (src.region && src.region[e] == 0) return false;
  *key = to_key(src.mode == kModeDeviation ? fabs(x - src.centre) : x);
  return true;
}

// f(valid, key) for every element, called by whole waves (every lane of a
// wave makes the same calls; lanes without an element pass valid = false)
template <typename F>
__device__ __forceinline__ void for_each_key(const SelectSource& src, F&& f) {
  const int64_t npairs = (src.n - src.head) / 2;
  const int64_t stride = (int64_t)gridDim.x * kSelThreads;
  const int64_t me = (int64_t)blockIdx.x * kSelThreads + threadIdx.x;
  for (int64_t i0 = 0; i0 < npairs; i0 += stride * kSelUnroll) {  // uniform
    u64 key[kSelUnroll][2];
    bool ok[kSelUnroll][2];
    if (src.keys) {
      ulonglong2 v[kSelUnroll];
#pragma unroll
      for (int k = 0; k < kSelUnroll; ++k) {
        const int64_t i = i0 + k * stride + me;
        ok[k][0] = ok[k][1] = i < npairs;
        v[k] = make_ulonglong2(0, 0);
        if (i < npairs) v[k] = reinterpret_cast<const ulonglong2*>(src.keys)[i];
      }
#pragma unroll
      for (int k = 0; k < kSelUnroll; ++k) key[k][0] = v[k].x, key[k][1] = v[k].y;
    } else {
      double2 v[kSelUnroll];
#pragma unroll
      for (int k = 0; k < kSelUnroll; ++k) {
        const int64_t i = i0 + k * stride + me;
        v[k] = make_double2(0.0, 0.0);
        if (i < npairs) v[k] = reinterpret_cast<const double2*>(src.img + src.head)[i];
      }
#pragma unroll
      for (int k = 0; k < kSelUnroll; ++k) {
        const int64_t i = i0 + k * stride + me;
        const int64_t e = src.head + 2 * i;
        key[k][0] = key[k][1] = 0;
        ok[k][0] = i < npairs && sample_key(src, v[k].x, e, &key[k][0]);
        ok[k][1] = i < npairs && sample_key(src, v[k].y, e + 1, &key[k][1]);
      }
    }
#pragma unroll
    for (int k = 0; k < kSelUnroll; ++k) {
      f(ok[k][0], key[k][0]);
      f(ok[k][1], key[k][1]);
    }
  }
  // the loose elements: element 0 before the first pair, the last one behind the last pair
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    int64_t e = -1;
    if (threadIdx.x == 0 && src.head) e = 0;
    if (threadIdx.x == 1 && ((src.n - src.head) & 1)) e = src.n - 1;
    u64 key = 0;
    bool ok = false;
    if (e >= 0) {
      if (src.keys) {
        key = src.keys[e];
        ok = true;
      } else {
        ok = sample_key(src, src.img[e], e, &key);
      }
    }
    f(ok, key);
  }
}

// s_hist[digit] += 1 for every active lane, with one add per distinct digit of
// the wave: `bits` ballots give every lane the set of active lanes that hold
// its digit, and the lowest lane of each set adds the set's size
__device__ __forceinline__ void wave_add(unsigned* s_hist, bool active, unsigned digit, int bits) {
  u64 peers = __ballot(active);
  if (peers == 0) return;  // uniform: no lane matches the prefix
  for (int b = 0; b < bits; ++b) {  // uniform
    const bool one = (digit >> b) & 1u;
    const u64 m = __ballot(one);
    peers &= one ? m : ~m;
  }
  const int lane = threadIdx.x & 63;
  if (active && (peers & (((u64)1 << lane) - 1)) == 0) atomicAdd(&s_hist[digit], (unsigned)__popcll(peers));
}

// part[block][bin]: the block's count of samples that match (himask, prefix), by the digit at `shift`
__global__ __launch_bounds__(kSelThreads) void select_hist_kernel(SelectSource src, u64 himask, u64 prefix, int shift,
                                                                  int bits, unsigned* __restrict__ part) {
  __shared__ unsigned s_hist[kSelMaxBins];
  const int nbins = 1 << bits;
  for (int b = threadIdx.x; b < nbins; b += kSelThreads) s_hist[b] = 0u;
  __syncthreads();
  const unsigned dmask = (unsigned)nbins - 1u;
  for_each_key(src, [&](bool ok, u64 key) {
    wave_add(s_hist, ok && (key & himask) == prefix, (unsigned)(key >> shift) & dmask, bits);
  });
  __syncthreads();
  unsigned* row = part + (int64_t)blockIdx.x * nbins;
  for (int b = threadIdx.x; b < nbins; b += kSelThreads) row[b] = s_hist[b];
}

// hist[bin] = sum over the blocks' rows: a workgroup takes 64 bins, its four waves a quarter of the rows each
__global__ __launch_bounds__(256) void select_reduce_kernel(const unsigned* __restrict__ part, int nblocks, int nbins,
                                                            u64* __restrict__ hist) {
  __shared__ u64 s_sum[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + lane;  // < nbins: a multiple of 64
  u64 sum = 0;
  for (int r = wave; r < nblocks; r += 4) sum += part[(int64_t)r * nbins + b];
  s_sum[wave][lane] = sum;
  __syncthreads();
  if (wave == 0) hist[b] = s_sum[0][lane] + s_sum[1][lane] + s_sum[2][lane] + s_sum[3][lane];
}

// one block: the bin that holds the rank; prefix, rank and ncand move on to it
__global__ __launch_bounds__(256) void select_scan_kernel(const u64* __restrict__ hist, int nbins, int shift, int first,
                                                          SelectState* __restrict__ st) {
  __shared__ u64 s_part[256];
  const int per = nbins / 256;
  u64 sum = 0;
  for (int b = threadIdx.x * per; b < (threadIdx.x + 1) * per; ++b) sum += hist[b];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  u64 total = 0;
  for (int t = 0; t < 256; ++t) total += s_part[t];
  long long rank = st->rank;
  if (first) {
    st->count = (long long)total;
    if (rank < 0) rank = total ? (long long)((total - 1) / 2) : 0;
  }
  if ((u64)rank >= total) {
    st->status = 1;
    st->ncand = 0;
    return;
  }
  u64 below = 0;
  int t = 0;
  while (below + s_part[t] <= (u64)rank) below += s_part[t++];
  int b = t * per;
  while (below + hist[b] <= (u64)rank) below += hist[b++];
  st->prefix |= (u64)b << shift;
  st->rank = rank - (long long)below;
  st->ncand = (long long)hist[b];
}

// the keys of the samples that match (himask, prefix), in any order
__global__ __launch_bounds__(kSelThreads) void select_compact_kernel(SelectSource src, u64 himask, u64 prefix,
                                                                     u64* __restrict__ keys_out, int64_t cap,
                                                                     SelectState* __restrict__ st) {
  const int lane = threadIdx.x & 63;
  for_each_key(src, [&](bool ok, u64 key) {
    const bool take = ok && (key & himask) == prefix;
    const u64 m = __ballot(take);
    if (m == 0) return;  // uniform
    const int leader = __ffsll((long long)m) - 1;
    u64 base = 0;
    if (lane == leader) base = atomicAdd(&st->nkeys, (u64)__popcll(m));
    base = (u64)__shfl((long long)base, leader);
    const u64 pos = base + (u64)__popcll(m & (((u64)1 << lane) - 1));
    if (take && pos < (u64)cap) keys_out[pos] = key;  // the histogram counted them: they fit
  });
}

int select_blocks(int64_t n) {
  const int64_t per = (int64_t)kSelThreads * kSelUnroll * 2;
  const int64_t b = (n + per - 1) / per;
  return (int)(b < 1 ? 1 : b > kSelMaxBlocks ? kSelMaxBlocks : b);
}

// One select on stream s: the sample of `rank` (< 0: the lower median) among
// the keys of `mode`. *found false: the rank lies outside the samples (none at
// all included). Blocks until the value is on the host.
int select_run(Workspace* ws, hipStream_t s, const double* img, int64_t n, const uint8_t* region, int mode,
               double centre, int64_t rank, int64_t* count, double* value, bool* found) {
  CIP_ALLOC(part, unsigned, "noise_part", (int64_t)kSelMaxBlocks * kSelMaxBins)
  CIP_ALLOC(hist, u64, "noise_hist", kSelMaxBins)
  CIP_ALLOC(keys, u64, "noise_keys", kCompactCap)
  CIP_ALLOC(state, SelectState, "noise_state", 1)
  SelectState* h = (SelectState*)pinned(ws, sizeof(SelectState));
  if (!h) return CIP_ENOMEM;
  *h = SelectState{0, (long long)rank, 0, 0, 0, 0};
  // the staging (the readbacks' own) is next written by the first pass's readback, behind this copy on the stream
  CIP_HIP_CHECK(hipMemcpyAsync(state, h, sizeof(SelectState), hipMemcpyHostToDevice, s));
  SelectSource src{img, region, nullptr, n, (int64_t)(((uintptr_t)img & 15u) ? 1 : 0), mode, centre};
  u64 himask = 0, prefix = 0;
  int shift = 64;
  for (int pass = 0; pass < kSelPasses; ++pass) {
    const int nbins = 1 << kSelBits[pass];
    shift -= kSelBits[pass];
    const int blocks = select_blocks(src.n);
    select_hist_kernel<<<dim3(blocks), dim3(kSelThreads), 0, s>>>(src, himask, prefix, shift, kSelBits[pass], part);
    CIP_HIP_CHECK(hipGetLastError());
    select_reduce_kernel<<<dim3(nbins / 64), dim3(256), 0, s>>>(part, blocks, nbins, hist);
    CIP_HIP_CHECK(hipGetLastError());
    select_scan_kernel<<<dim3(1), dim3(256), 0, s>>>(hist, nbins, shift, pass == 0, state);
    CIP_HIP_CHECK(hipGetLastError());
    if (const int rc = readback(ws, s, {{state, sizeof(SelectState)}}, &h); rc != CIP_OK) return rc;
    if (pass == 0) *count = h->count;
    if (h->status) {
      *found = false;
      *value = std::nan("");
      return CIP_OK;
    }
    prefix = h->prefix;
    himask |= (u64)(nbins - 1) << shift;
    if (!src.keys && pass + 1 < kSelPasses && h->ncand <= kCompactCap) {
      select_compact_kernel<<<dim3(blocks), dim3(kSelThreads), 0, s>>>(src, himask, prefix, keys, kCompactCap, state);
      CIP_HIP_CHECK(hipGetLastError());
      src = SelectSource{nullptr, nullptr, keys, (int64_t)h->ncand, 0, kModeValue, 0.0};
    }
  }
  *found = true;
  *value = from_key(prefix);
  return CIP_OK;
}

int image_check(const std::string& who, const double* image, int64_t nx, int64_t ny) {
  if (!image) return set_error(CIP_EINVAL, who + ": image must not be NULL");
  if (nx < 1 || ny < 1) return set_error(CIP_EINVAL, who + ": image dimensions must be >= 1");
  if (nx > INT64_MAX / ny) return set_error(CIP_EINVAL, who + ": image too large");
  return CIP_OK;
}

int image_select_impl(const double* image, int64_t nx, int64_t ny, const uint8_t* region, int64_t rank,
                      void* hip_stream, int64_t* count_out, double* value_out) {
  const std::string who = "cip_image_select";
  if (const int rc = image_check(who, image, nx, ny); rc != CIP_OK) return rc;
  if (!count_out || !value_out) return set_error(CIP_EINVAL, who + ": count_out and value_out must not be NULL");
  if (rank < 0) return set_error(CIP_EINVAL, who + ": rank must be >= 0");
  CIP_BEGIN_CALL(hip_stream, false)
  bool found = false;
  if (const int rc = select_run(ws, s, image, nx * ny, region, kModeValue, 0.0, rank, count_out, value_out, &found);
      rc != CIP_OK)
    return rc;
  if (!found)
    return set_error(CIP_ERANGE, who + ": rank " + std::to_string(rank) + " is not below the " +
                                     std::to_string(*count_out) + " samples");
  return CIP_OK;
}

int image_noise_impl(const double* image, int64_t nx, int64_t ny, const uint8_t* region, void* hip_stream,
                     cip_noise_result* out) {
#pragma clang fp contract(off)
  const std::string who = "cip_image_noise";
  if (const int rc = image_check(who, image, nx, ny); rc != CIP_OK) return rc;
  if (!out) return set_error(CIP_EINVAL, who + ": out must not be NULL");
  CIP_BEGIN_CALL(hip_stream, false)
  bool found = false;
  out->count = 0;
  out->median = out->mad = out->sigma = std::nan("");
  if (const int rc = select_run(ws, s, image, nx * ny, region, kModeValue, 0.0, -1, &out->count, &out->median, &found);
      rc != CIP_OK)
    return rc;
  if (!found) return CIP_OK;  // no samples
  int64_t count = 0;
  if (const int rc = select_run(ws, s, image, nx * ny, region, kModeDeviation, out->median, -1, &count, &out->mad,
                                &found);
      rc != CIP_OK)
    return rc;
  if (!found || count != out->count) return set_error(CIP_EHIP, who + ": the two selects disagree on the samples");
  out->sigma = CIP_MAD_TO_SIGMA * out->mad;
  return CIP_OK;
}

// --------------------------------------------------------------- mask ----
constexpr int kMaskThreads = 256;
constexpr int kMaskTX = 32, kMaskTY = 64;  // a tile: 32 rows of 64 adjacent pixels, one column per lane
constexpr int kMaskRows = kMaskTX / (kMaskThreads / 64);  // rows of a column one thread owns
constexpr int kMaskPitch = kMaskTY + 4;
constexpr int kMaskRoundsPerCheck = 8;  // rounds queued between two reads of their flags
constexpr int kMaskMaxBlocks = 4096;    // the grids of the two element-wise kernels
static_assert(kMaskTY == 64 && kMaskRows * (kMaskThreads / 64) == kMaskTX, "a wave is one row of a tile");
constexpr uint8_t kOut = 0, kCand = 1, kIn = 2;

struct MaskSmall {
  u64 n_seed, n_island, n_out;
  unsigned changed[kMaskRoundsPerCheck];
};

// the wave's sum of v, added to *dst by one lane
__device__ __forceinline__ void wave_count(u64* dst, unsigned v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (u64)v);
}

__global__ __launch_bounds__(kMaskThreads) void mask_init_kernel(const double* __restrict__ img, int64_t n,
                                                                 double seed, double grow,
                                                                 const uint8_t* __restrict__ region, int positive,
                                                                 uint8_t* __restrict__ state, int64_t ny,
                                                                 int64_t ntx, int64_t nty,
                                                                 uint8_t* __restrict__ dirty,
                                                                 MaskSmall* __restrict__ small) {
  unsigned seeds = 0;
  for (int64_t p = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kMaskThreads) {
    const double x = img[p], a = positive ? x : fabs(x);
    uint8_t st = kOut;
    if ((!region || region[p] != 0) && a >= grow) st = a >= seed ? kIn : kCand;  // NaN: neither
    state[p] = st;
    if (st == kIn) {  // the first round takes the tiles that see a seed: its own, and across an edge it lies on
      const int64_t i = p / ny, j = p % ny, ti = i / kMaskTX, tj = j / kMaskTY;
      const int ri = (int)(i % kMaskTX), rj = (int)(j % kMaskTY);
      for (int64_t ta = ti - (ri == 0); ta <= ti + (ri == kMaskTX - 1); ++ta)
        for (int64_t tb = tj - (rj == 0); tb <= tj + (rj == kMaskTY - 1); ++tb)
          if (ta >= 0 && ta < ntx && tb >= 0 && tb < nty) dirty[ta * nty + tb] = 1;
    }
    seeds += st == kIn;
  }
  wave_count(&small->n_seed, seeds);
}

__global__ __launch_bounds__(kMaskThreads) void mask_round_kernel(uint8_t* state, int64_t nx, int64_t ny, int64_t nty,
                                                                  int conn4, uint8_t* dirty, uint8_t* dirty_next,
                                                                  unsigned* changed) {
  __shared__ uint8_t s_raw[(kMaskTX + 2) * kMaskPitch];
  if (!dirty[blockIdx.x]) return;  // uniform: nothing this tile sees has changed since it was last stable
  volatile uint8_t* s = s_raw;  // neighbours are written by other lanes between two barriers
  const int64_t i0 = ((int64_t)blockIdx.x / nty) * kMaskTX, j0 = ((int64_t)blockIdx.x % nty) * kMaskTY;
  for (int c = threadIdx.x; c < (kMaskTX + 2) * (kMaskTY + 2); c += kMaskThreads) {
    const int r = c / (kMaskTY + 2), q = c % (kMaskTY + 2);
    const int64_t i = i0 - 1 + r, j = j0 - 1 + q;
    s[r * kMaskPitch + q] = (i >= 0 && i < nx && j >= 0 && j < ny) ? state[i * ny + j] : kOut;
  }
  __syncthreads();
  if (threadIdx.x == 0) dirty[blockIdx.x] = 0;  // every thread has read it; the round after next reuses the array
  const int col = (threadIdx.x & 63) + 1, r0 = (threadIdx.x >> 6) * kMaskRows + 1;
  unsigned cand = 0;  // bit k: row r0 + k of this column is a candidate
#pragma unroll
  for (int k = 0; k < kMaskRows; ++k) cand |= (unsigned)(s[(r0 + k) * kMaskPitch + col] == kCand) << k;
  if (!__syncthreads_or(cand != 0)) return;  // nothing in the tile can change
  const auto touches = [&](int r) {
    const volatile uint8_t* c = s + r * kMaskPitch + col;
    bool t = c[-kMaskPitch] == kIn || c[kMaskPitch] == kIn || c[-1] == kIn || c[1] == kIn;
    if (!conn4)
      t = t || c[-kMaskPitch - 1] == kIn || c[-kMaskPitch + 1] == kIn || c[kMaskPitch - 1] == kIn ||
          c[kMaskPitch + 1] == kIn;
    return t;
  };
  unsigned turned = 0;
  for (;;) {
    unsigned now = 0;
    // down the column and up again, so a vertical run is one step
    for (int k = 0; k < kMaskRows; ++k)
      if (((cand & ~turned & ~now) >> k) & 1u)
        if (touches(r0 + k)) s[(r0 + k) * kMaskPitch + col] = kIn, now |= 1u << k;
    for (int k = kMaskRows - 2; k >= 0; --k)
      if (((cand & ~turned & ~now) >> k) & 1u)
        if (touches(r0 + k)) s[(r0 + k) * kMaskPitch + col] = kIn, now |= 1u << k;
    turned |= now;
    if (!__syncthreads_or(now != 0)) break;
  }
  // a candidate lies inside the image, so a turned pixel does
  for (int k = 0; k < kMaskRows; ++k)
    if ((turned >> k) & 1u) state[(i0 + r0 - 1 + k) * ny + (j0 + col - 1)] = kIn;
  if (__syncthreads_or(turned != 0) && threadIdx.x == 0) {
    *changed = 1u;
    // the eight tiles whose halo this one touches look again in the next round; this tile is stable until
    // one of them changes
    const int64_t ti = (int64_t)blockIdx.x / nty, tj = (int64_t)blockIdx.x % nty, ntx = (int64_t)gridDim.x / nty;
    for (int64_t a = ti - 1; a <= ti + 1; ++a)
      for (int64_t b = tj - 1; b <= tj + 1; ++b)
        if ((a != ti || b != tj) && a >= 0 && a < ntx && b >= 0 && b < nty) dirty_next[a * nty + b] = 1;
  }
}

// mask_out may be base: a thread reads base[p] before it writes mask_out[p]
__global__ __launch_bounds__(kMaskThreads) void mask_final_kernel(const uint8_t* __restrict__ state,
                                                                  const uint8_t* base, int64_t n, uint8_t* mask_out,
                                                                  MaskSmall* __restrict__ small) {
  unsigned island = 0, ones = 0;
  for (int64_t p = (int64_t)blockIdx.x * kMaskThreads + threadIdx.x; p < n; p += (int64_t)gridDim.x * kMaskThreads) {
    const bool in = state[p] == kIn;
    const bool one = in || (base && base[p] != 0);
    mask_out[p] = one ? 1 : 0;
    island += in;
    ones += one;
  }
  wave_count(&small->n_island, island);
  wave_count(&small->n_out, ones);
}

int auto_mask_impl(const double* image, int64_t nx, int64_t ny, double seed, double grow, const uint8_t* region,
                   const uint8_t* base, int flags, void* hip_stream, uint8_t* mask_out, cip_mask_result* out) {
  const std::string who = "cip_auto_mask";
  if (const int rc = image_check(who, image, nx, ny); rc != CIP_OK) return rc;
  if (!mask_out || !out) return set_error(CIP_EINVAL, who + ": mask_out and out must not be NULL");
  if (!std::isfinite(seed) || !std::isfinite(grow) || !(grow > 0.0) || !(seed >= grow))
    return set_error(CIP_EINVAL, who + ": seed and grow must be finite with seed >= grow > 0");
  if (flags & ~(CIP_MASK_POSITIVE | CIP_MASK_CONN4)) return set_error(CIP_EINVAL, who + ": unknown flag bits");
  const int64_t ntx = (nx + kMaskTX - 1) / kMaskTX, nty = (ny + kMaskTY - 1) / kMaskTY;
  if (ntx > (((int64_t)1 << 31) - 1) / nty) return set_error(CIP_EINVAL, who + ": image has 2^31 tiles or more");
  const int64_t n = nx * ny;
  CIP_BEGIN_CALL(hip_stream, false)
  CIP_ALLOC(state, uint8_t, "mask_state", n)
  CIP_ALLOC(dirty, uint8_t, "mask_tiles", 2 * ntx * nty)  // the tiles a round works on, and the next round's
  CIP_ALLOC(small, MaskSmall, "mask_small", 1)
  MaskSmall* h = nullptr;
  const int64_t want = (n + kMaskThreads - 1) / kMaskThreads;
  const int blocks = (int)(want > kMaskMaxBlocks ? kMaskMaxBlocks : want);
  CIP_HIP_CHECK(hipMemsetAsync(small, 0, sizeof(MaskSmall), s));
  CIP_HIP_CHECK(hipMemsetAsync(dirty, 0, (size_t)(2 * ntx * nty), s));
  mask_init_kernel<<<dim3(blocks), dim3(kMaskThreads), 0, s>>>(image, n, seed, grow, region,
                                                               flags & CIP_MASK_POSITIVE, state, ny, ntx, nty, dirty, small);
  CIP_HIP_CHECK(hipGetLastError());
  int64_t rounds = 0;
  for (;;) {  // until a round changes nothing: no cap (a serpentine island needs many)
    CIP_HIP_CHECK(hipMemsetAsync(small->changed, 0, sizeof(small->changed), s));
    for (int q = 0; q < kMaskRoundsPerCheck; ++q) {
      mask_round_kernel<<<dim3((unsigned)(ntx * nty)), dim3(kMaskThreads), 0, s>>>(state, nx, ny, nty,
                                                                                   flags & CIP_MASK_CONN4,
                                                                                   dirty + ((rounds + q) & 1) * ntx * nty,
                                                                                   dirty + ((rounds + q + 1) & 1) * ntx * nty,
                                                                                   small->changed + q);
      CIP_HIP_CHECK(hipGetLastError());
    }
    rounds += kMaskRoundsPerCheck;
    if (const int rc = readback(ws, s, {{small, sizeof(MaskSmall)}}, &h); rc != CIP_OK) return rc;
    if (!h->changed[kMaskRoundsPerCheck - 1]) break;  // and so would every later round
  }
  mask_final_kernel<<<dim3(blocks), dim3(kMaskThreads), 0, s>>>(state, base, n, mask_out, small);
  CIP_HIP_CHECK(hipGetLastError());
  if (const int rc = readback(ws, s, {{small, sizeof(MaskSmall)}}, &h); rc != CIP_OK) return rc;
  out->n_seed = (int64_t)h->n_seed;
  out->n_island = (int64_t)h->n_island;
  out->n_out = (int64_t)h->n_out;
  out->rounds = rounds;
  return CIP_OK;
}

}  // namespace

}  // namespace cip

using namespace cip;

extern "C" {

int cip_image_select(const double* image, int64_t nx, int64_t ny, const uint8_t* region, int64_t rank,
                     void* hip_stream, int64_t* count_out, double* value_out) {
  clear_error();
  return image_select_impl(image, nx, ny, region, rank, hip_stream, count_out, value_out);
}

int cip_image_noise(const double* image, int64_t nx, int64_t ny, const uint8_t* region, void* hip_stream,
                    cip_noise_result* out) {
  clear_error();
  return image_noise_impl(image, nx, ny, region, hip_stream, out);
}

int cip_auto_mask(const double* image, int64_t nx, int64_t ny, double seed, double grow, const uint8_t* region,
                  const uint8_t* base, int flags, void* hip_stream, uint8_t* mask_out, cip_mask_result* out) {
  clear_error();
  return auto_mask_impl(image, nx, ny, seed, grow, region, base, flags, hip_stream, mask_out, out);
}

}  // extern "C"

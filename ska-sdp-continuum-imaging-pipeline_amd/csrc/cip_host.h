// cip_host.h - what the host-side units of libcip_hip.so share (cip_workspace,
// cip_params, cip_planner, cip_invert, cip_predict and the entry points kept
// beside their launchers in cip_clean, cip_strips, cip_tiling): the per-thread
// workspace with its cached host tables (host_table), its one readback
// (readback), the grid's known-zero state (GridZero) and the plan pipeline
// (PlanPipeline, PlanScope), the planner's request and result, the call scope
// that closes itself (Call) and the CIP_* switches. Host only and not part of
// the C ABI (include/cip.h is); units that hold nothing but kernels and
// launchers include cip_internal.h alone.
#pragma once
#include <hipfft/hipfft.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "cip_internal.h"

namespace cip {

// ----------------------------------------------------------- profiler ----
// hipEvents recorded on the call's stream around each phase (cip_profile_*).
struct Profiler {
  bool on = false;
  int device = -1;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  struct Span {
    int phase;
    hipEvent_t a, b;
  };
  std::vector<Span> spans;
  double ms[CIP_PROFILE_PHASES] = {0};
  int64_t counts[CIP_PROFILE_COUNTS] = {0};

  void reset() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev != device) {  // events belong to a device
      for (auto e : pool) (void)hipEventDestroy(e);
      pool.clear();
      device = dev;
    }
    used = 0;
    spans.clear();
    for (auto& m : ms) m = 0.0;
    for (auto& c : counts) c = 0;
  }
  hipEvent_t mark(hipStream_t s) {
    if (!on) return nullptr;
    if (used == pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      pool.push_back(e);
    }
    hipEvent_t e = pool[used++];
    if (hipEventRecord(e, s) != hipSuccess) return nullptr;
    return e;
  }
  void span(int phase, hipEvent_t a, hipEvent_t b) {
    if (on && a && b) spans.push_back({phase, a, b});
  }
  void finish() {  // stream already synchronised
    if (!on) return;
    for (auto& sp : spans) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) ms[sp.phase] += t;
    }
  }
};
extern thread_local Profiler g_prof;  // cip_workspace.hip

// ---------------------------------------------------------- workspace ----
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
};

struct FftPlan {
  hipfftHandle h;
  int64_t nu, nv;
};

struct PlanResult {
  int64_t nruns = 0, ntiles = 0, nchunks = 0;
  std::vector<int64_t> plane_chunk_off;  // chunk offset of each range: w plane group q (ngroups + 1), or the 2-D layer
  int group = 1;                         // w planes per work unit (w-stacking plane groups)
  uint64_t* runs = nullptr;
  int64_t* run_goff = nullptr;
  int64_t* tile_run_off = nullptr;
  Chunk* chunks = nullptr;
  void* perm = nullptr;  // bank-class ordered visibility stream (perm_encode entries), or NULL
  bool phases = false;   // perm's entries carry row phases (RowMap::row_phase for the scatter)
  uint32_t* dmask = nullptr;  // 32-cell grid tiles the scatter writes, per plane (bit-packed, mtx / 32 words per tile row)
  int tx_shift = kTileShift, ty_shift = kTileShift;  // the work tile the plan was made on (GridGeometry's)
};

// A table the host computes and keeps on the device (host_table): the
// grid-correction vectors, the w-correction table, the FFT twiddles of each
// length, the restore taps and the multiscale taps.
struct HostTable {
  std::vector<double> key;  // what the device copy was made from; empty: none
  void* staging = nullptr;  // pinned, this table's own (every readback rewrites `pinned`); grows like it
  size_t staging_bytes = 0;
  hipEvent_t uploaded = nullptr;  // behind the last upload: the next one waits for it before it refills the staging
};

// The "grid" buffer's known-zero prefix (the masked FFT pass A zeroes what the
// scatter wrote). A byte count, not a plane count: a call on a smaller grid
// keeps only its own planes' bytes clean, and a larger one must not trust more.
struct GridZero {
  const void* grid_clean = nullptr;  // the buffer, or NULL: nothing is known
  size_t grid_clean_bytes = 0;       // how many of its leading bytes are zero
  size_t prefix(const void* p) const { return p == grid_clean ? grid_clean_bytes : 0; }
  bool covers(const void* p, size_t n) const { return p && prefix(p) >= n; }  // the first n bytes of p count as zero
  void mark(const void* p, size_t n) { *this = {p, std::max(prefix(p), n)}; }  // a larger prefix of the buffer stays
  void invalidate() { *this = GridZero(); }  // also when the buffer is reallocated (grid_buffer)
};

// CIP_ASYNC | CIP_PIPELINE (cip_ms2dirty): consecutive calls alternate between
// two sets of planner buffers (parity; buf() appends it to buffer names while
// a PlanScope plans), so the planner of call k + 1 runs on a plan stream
// beside call k's scatter and FFT; it only waits for call k - 1's work on the
// caller's stream (ev_done[parity]: its scatter read the plan, its FFT the
// masks and weight sum). One plan stream per parity. Only these methods and
// PlanScope (cip_workspace.hip) touch the fields.
struct PlanPipeline {
  hipStream_t plan_stream = nullptr, plan_stream1 = nullptr;
  hipEvent_t ev_done[2] = {nullptr, nullptr}, ev_planned = nullptr, ev_entry = nullptr;
  int parity = 0;
  bool parity_scope = false;
  bool plan_unscoped = false;  // a planner used the parity-0 names on a caller's stream since the last pipelined call

  bool odd_names() const { return parity_scope && parity; }  // buf_bytes: names carry "~1"
  void planner_starts() { plan_unscoped = plan_unscoped || !parity_scope; }  // prepare()
  void rewind() { parity = 0; }  // cip_dirty2ms plans into the parity-0 buffers and leaves the next invert there
  void destroy();                // drains and destroys the streams and events
};

// One invert's hold on the pipeline, in the order every return path keeps:
// open -> the planner on ps, buf() names carrying the parity -> join (plain
// names again; s waits for ev_planned, once, also after a failed plan) ->
// ~PlanScope (joins if nobody did, then records ev_done[parity] on s, behind
// everything the call queued there: the next planner of this parity waits for
// it). A call that is not pipelined plans on s: all of it no-ops.
struct PlanScope {
  PlanPipeline& pl;
  const hipStream_t s;
  hipStream_t ps = s;  // where the planner runs
  bool armed = false, joined = true;
  // pipelined: streams and events on first use, the plan streams wait for s if
  // plan_unscoped, the parity flips, ps waits for ev_done[parity]; else parity 0
  int open(bool pipelined);
  int join();
  ~PlanScope();
};

struct Workspace {
  int device = 0;  // the device every buffer, stream and event belongs to
  std::map<std::string, DevBuf> bufs;
  std::map<std::string, HostTable> tables;  // by name, as bufs
  std::vector<FftPlan> plans;
  void* pinned = nullptr;  // small host staging: what the last readback (or pinned()) handed out
  size_t pinned_bytes = 0;
  // second stream: zeroes the first grid plane while the planner runs
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  GridZero grid_zero;
  PlanPipeline pipeline;
  // the last call left work queued on async_stream (~Call): a call on another stream first waits for it
  bool async_queued = false;
  hipStream_t async_stream = nullptr;
  // the last complete plan (its buffers stay untouched until the next planner
  // runs) and the geometry it was made for: CIP_REUSE_PLAN calls with the
  // same key grid through it. Cleared when a planner starts; never set for
  // ragged rows (their row map lives in per-call buffers).
  bool saved_valid = false;
  std::vector<double> saved_key;
  cip_gridder_params saved_p;
  PlanResult saved_plan;
};

// ---- cip_workspace.hip ----
void clear_error();
// grow-only device buffer; returns nullptr (and sets the error) on failure
void* buf_bytes(Workspace* ws, const char* name, size_t bytes);
template <typename T>
T* buf(Workspace* ws, const char* name, int64_t count) {
  return (T*)buf_bytes(ws, name, (size_t)(count > 0 ? count : 1) * sizeof(T));
}
// the uv grid ("grid", never parity-named); growing it invalidates grid_zero
double* grid_buffer(Workspace* ws, size_t bytes);
#define CIP_ALLOC(var, T, name, n)  \
  T* var = buf<T>(ws, name, (n));   \
  if (!var) return CIP_ENOMEM;
// small pinned host staging; returns nullptr (and sets the error) on failure.
// A larger request frees and reallocates it: the pointer holds until the next
// pinned() or readback() on the workspace, so no function passes it on.
void* pinned(Workspace* ws, size_t bytes);
// A few scalars back on the host: sizes the staging once, copies every source
// into consecutive 8-byte-aligned slots of it (a NULL source leaves its slot
// unwritten), waits for s once. *host: the staging, under pinned()'s rule.
struct DevSrc {
  const void* dev;
  size_t bytes;
};
int readback_bytes(Workspace* ws, hipStream_t s, std::initializer_list<DevSrc> src, void** host);
template <typename T>
int readback(Workspace* ws, hipStream_t s, std::initializer_list<DevSrc> src, T** host) {
  return readback_bytes(ws, s, src, (void**)host);
}
// The two halves of host_table. open: *staging = NULL when the device copy was
// made from `key`; else forgets the key, waits for the last upload to have read
// the staging and hands out `bytes` of it. upload: staging -> dev on s, the
// event behind it, and only then the key.
int host_table_open(Workspace* ws, const char* name, const std::vector<double>& key, size_t bytes, void** staging);
int host_table_upload(Workspace* ws, const char* name, const std::vector<double>& key, void* dev, size_t bytes,
                      hipStream_t s);
// dev: the table's device buffer (a CIP_ALLOC of the caller's), used in stream
// order on s. Unless it was made from `key`: fill(staging), `bytes` to dev on
// s. Never waits for the stream: a call on another stream waits in begin_call
// for whatever this one leaves queued.
template <typename Fill>
int host_table(Workspace* ws, const char* name, const std::vector<double>& key, void* dev, size_t bytes,
               hipStream_t s, Fill&& fill) {
  void* staging = nullptr;
  if (const int rc = host_table_open(ws, name, key, bytes, &staging); rc != CIP_OK || !staging) return rc;
  fill(staging);
  return host_table_upload(ws, name, key, dev, bytes, s);
}
int fft_plan(Workspace* ws, int64_t nu, int64_t nv, hipStream_t s, hipfftHandle* out);
int fft_twiddles(Workspace* ws, int64_t n, hipStream_t s, double** out);
int zero_on_side(Workspace* ws, void* p, size_t bytes, hipStream_t s);
int join_side(Workspace* ws, hipStream_t s);

// One entry-point call: its workspace and stream, and (profiled calls) the
// event that starts span 5, the whole call. The scope closes itself: unless
// end_call waited for the stream, ~Call notes it in the workspace on every
// return path, so a later call on another stream waits for it in begin_call.
struct Call {
  Workspace* ws = nullptr;
  hipStream_t s = nullptr;
  bool profiled = false;
  hipEvent_t t0 = nullptr;
  bool synced = false;  // end_call waited for s: nothing of this call is queued
  Call() = default;
  Call(const Call&) = delete;
  Call& operator=(const Call&) = delete;
  ~Call();
};
// Clears the thread's error, takes its workspace (which arms the reaper, so
// argument checks come first), waits for an earlier call's work queued on
// another stream; profiled: resets the profiler and marks the start.
int begin_call(void* hip_stream, bool profiled, Call* c);
// Closes span 5; wait (or a profile to read): synchronises the stream and reads
// the profile; else the work stays queued (CIP_ASYNC) and ~Call notes the stream.
int end_call(Call& c, bool wait = true);
// the usual opening of an entry point, after its argument checks: declares
// `call`, and `ws` and `s` as the bodies (and CIP_ALLOC) name them
#define CIP_BEGIN_CALL(hip_stream, profiled)                                              \
  Call call;                                                                              \
  if (const int rc_ = begin_call(hip_stream, profiled, &call); rc_ != CIP_OK) return rc_; \
  Workspace* const ws = call.ws;                                                          \
  const hipStream_t s = call.s;                                                           \
  (void)ws;

// ---- cip_params.hip ----
int choose(int64_t npix_x, int64_t npix_y, double px, double py, double epsilon, int support, int do_wstacking,
           double wmin, double wmax, cip_gridder_params* out);
// the scatter's work tile as shifts (GridGeometry::tx_shift / ty_shift); 32 x 32 by default
struct TileShape {
  int tx_shift = kTileShift, ty_shift = kTileShift;
};
// the larger work tile of the selection rule (scatter_tile_shape)
constexpr TileShape kDefaultScatterTile{6, 6};
GridGeometry geometry(const cip_gridder_params& p, double px, double py, TileShape t = TileShape());
TileShape scatter_tile_shape(const cip_gridder_params& p, bool packed, bool eligible);
int correction_vectors(Workspace* ws, const GridGeometry& g, int64_t npix_x, int64_t npix_y, hipStream_t s,
                       double** cx_out, double** cy_out);
int w_correction_table(Workspace* ws, const cip_gridder_params& prm, const GridGeometry& g, hipStream_t s,
                       double** table, int64_t* n, double* dnu_out);
int wstack_group(const GridGeometry& g, bool packed);
bool grid_is_transposed(const GridGeometry& g, int64_t npix_x, int64_t npix_y);
bool vis_dtype_ok(int d);
bool public_dtypes(int vis_dtype, int wgt_dtype);
int public_dtype_check(int vis_dtype, int wgt_dtype, bool any_vis);
// the CIP_* switches (one table in cip_params.hip; place_rows64,
// fft_f32_enabled and order_classes32 are declared in cip_internal.h)
bool fft_pruned();
bool grid_mask();
bool scatter_order();
bool packed_runs();
bool ragged_pack();
bool row_phases();
int wstack_group_cap();
int flush_store_mode();
int scatter_tile_force();
bool grid_f32_enabled();
bool wacc_f32_enabled();
bool fft_rowskip();
bool mosaic_lds();

struct Prepared {
  cip_gridder_params p;
  GridGeometry g;
  double fixed_scale;
  bool packed;  // single-precision class (CIP_ACC_SINGLE)
  double* fx;
  double* red;  // device [sum_w, max|wV|]
  RowMap m;     // (row, channel) -> visibility index
  PlanResult plan;
};

// Row slices of the ragged (tile) input layout: row r holds channels
// [chan_start[r], chan_stop[r]) and the visibilities are concatenated in row
// order (reference uvw_tiling/tile.py:83-115), nvis in total.
struct RaggedRows {
  const int32_t* chan_start;
  const int32_t* chan_stop;
  int64_t nvis;
};

// What prepare() plans for. given: fixed parameters (npix_x, npix_y and
// epsilon are then not consulted); plane_end >= 0: a range of the w-plane stack.
struct PlanRequest {
  const double *uvw = nullptr, *freq = nullptr;
  int64_t nrow = 0, nchan = 0;
  const void *vis = nullptr, *wgt = nullptr;
  int vis_dtype = CIP_C64, wgt_dtype = CIP_NONE;
  const uint8_t* flags4 = nullptr;
  int64_t npix_x = 0, npix_y = 0;
  double px = 0.0, py = 0.0, epsilon = 0.0;
  int support = 0, do_wstacking = 0;
  bool packed = false;
  const cip_gridder_params* given = nullptr;
  const RaggedRows* ragged = nullptr;
  bool reuse = false;      // CIP_REUSE_PLAN
  bool want_group = true;  // w-plane groups (wstack_group); false: one plane per work unit
  bool wide_tile = false;  // a cip_ms2dirty* call: the plan may use a larger work tile (scatter_tile_shape)
  int64_t plane_begin = 0, plane_end = -1;

  // What to plan for: an image and an accuracy,
  static PlanRequest image(int64_t npix_x, int64_t npix_y, double px, double py, double epsilon, int support) {
    PlanRequest rq;
    rq.npix_x = npix_x, rq.npix_y = npix_y, rq.px = px, rq.py = py, rq.epsilon = epsilon, rq.support = support;
    return rq;
  }
  // or given parameters (NULL: the caller reports it) and the call's flags. A dummy image size: the planner
  // then consults it for nothing but its CIP_REUSE_PLAN key, which a call with given parameters never matches.
  static PlanRequest fixed(const cip_gridder_params* params, double px, double py, int flags) {
    PlanRequest rq = image(2, 2, px, py, 0.0, params ? params->support : 0);
    rq.do_wstacking = params ? params->do_wstacking : 0;
    rq.packed = (flags & CIP_ACC_SINGLE) != 0;
    rq.given = params;
    return rq;
  }
  // of dense rows (ragged row slices: the caller then sets `ragged`),
  PlanRequest& dense(const double* uvw_, int64_t nrow_, const double* freq_, int64_t nchan_, const void* vis_,
                     int vis_dtype_, const void* wgt_, int wgt_dtype_) {
    uvw = uvw_, nrow = nrow_, freq = freq_, nchan = nchan_;
    vis = vis_, vis_dtype = vis_dtype_, wgt = wgt_, wgt_dtype = wgt_dtype_;
    return *this;
  }
  // raw linear-feed rows (CIP_POL4I),
  PlanRequest& raw(const double* uvw_, int64_t nrow_, const double* freq_, int64_t nchan_, const void* vis4,
                   const uint8_t* flags4_, const float* wgt4) {
    flags4 = flags4_;
    return dense(uvw_, nrow_, freq_, nchan_, vis4, CIP_POL4I, wgt4, CIP_POL4I);
  }
};

// prepare()'s decision about the workspace grid: an invert's first plane group.
// The packed class grids into complex64 planes on the pruned-FFT path (half
// the flush and pass-A bytes); CIP_GRID_F32=0 keeps complex128 (A/B)
inline bool grid_planes_f32(bool packed, const GridGeometry& g, int64_t npix_x, int64_t npix_y) {
  return packed && grid_is_transposed(g, npix_x, npix_y) && grid_f32_enabled();
}
struct GridUse {
  bool beside = false;  // in: the planner runs on the call's stream, so zero the group beside it (zero_on_side)
  double* grid = nullptr;
  size_t bytes = 0;      // of the group's planes in their cell type
  bool f32 = false;      // complex64 planes (grid_planes_f32)
  bool zeroed = false;   // the bytes count as zero: left clean by the last invert, or the side memset
  bool pending = false;  // the side memset is queued: the caller joins it (join_side) whatever happens
};
// cip_planner.hip. grid_out (may be NULL): also takes the workspace grid
int prepare(Workspace* ws, const PlanRequest& rq, hipStream_t s, Prepared* out, GridUse* grid_out = nullptr);

}  // namespace cip

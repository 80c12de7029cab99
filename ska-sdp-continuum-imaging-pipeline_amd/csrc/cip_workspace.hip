// cip_workspace.hip - per-thread state of the host API: the error string, the
// profiler, the (device, thread) workspace with its buffers, cached host
// tables, readback staging, FFT plans and side stream, and the call scope
// every entry point opens.
#include <cmath>
#include <mutex>
#include <thread>

#include "cip_host.h"

namespace cip {

static thread_local std::string g_last_error;

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

void clear_error() { g_last_error.clear(); }

thread_local Profiler g_prof;

static int settle_async(Workspace* ws, hipStream_t s) {
  hipStream_t prev = ws->async_stream;
  ws->async_stream = nullptr;
  if (prev && prev != s) CIP_HIP_CHECK(hipStreamSynchronize(prev));
  return CIP_OK;
}

// Zero `bytes` at `p` on the workspace's side stream, ordered after the work
// already queued on s; join_side() makes s wait for it.
int zero_on_side(Workspace* ws, void* p, size_t bytes, hipStream_t s) {
  if (!ws->side) {
    CIP_HIP_CHECK(hipStreamCreateWithFlags(&ws->side, hipStreamNonBlocking));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&ws->ev_fork, hipEventDisableTiming));
    CIP_HIP_CHECK(hipEventCreateWithFlags(&ws->ev_join, hipEventDisableTiming));
  }
  CIP_HIP_CHECK(hipEventRecord(ws->ev_fork, s));
  CIP_HIP_CHECK(hipStreamWaitEvent(ws->side, ws->ev_fork, 0));
  CIP_HIP_CHECK(hipMemsetAsync(p, 0, bytes, ws->side));
  CIP_HIP_CHECK(hipEventRecord(ws->ev_join, ws->side));
  ws->side_pending = true;
  return CIP_OK;
}

int join_side(Workspace* ws, hipStream_t s) {
  if (!ws->side_pending) return CIP_OK;
  ws->side_pending = false;
  CIP_HIP_CHECK(hipStreamWaitEvent(s, ws->ev_join, 0));
  return CIP_OK;
}

static std::mutex g_ws_mutex;
// One workspace per (device, host thread): calls from different threads (e.g.
// two inverts in flight on one GPU, each thread on its own stream) never
// share buffers, the side stream or the clean-grid state. A workspace holds
// the uv grid (16 nu nv bytes) and planner buffers that grow with the
// visibility count, so it lives only as long as its thread: a thread-exit hook
// frees the workspaces of every worker thread that made one (dask worker
// pools keep HBM use at one workspace per live thread), and
// cip_release_workspace frees the calling thread's on demand.
static std::map<std::pair<int, std::thread::id>, Workspace*> g_ws;
// the thread that loaded the library: its workspaces are left to process
// teardown (its thread-exit hook runs inside exit(), where the HIP runtime
// may already be shutting down)
static const std::thread::id g_load_thread = std::this_thread::get_id();

static void destroy_workspace(Workspace* ws) {
  // the workspace's device current while its buffers go (the reaper may run on
  // a thread whose current device differs), and a CIP_ASYNC call's work drained
  // first: its scatter / FFT may still be queued on the caller's stream
  int prev_dev = -1;
  (void)hipGetDevice(&prev_dev);
  if (prev_dev != ws->device) (void)hipSetDevice(ws->device);
  if (ws->async_stream) (void)hipStreamSynchronize(ws->async_stream);
  if (ws->plan_stream) (void)hipStreamSynchronize(ws->plan_stream);
  if (ws->plan_stream1) (void)hipStreamSynchronize(ws->plan_stream1);
  for (auto& kv : ws->bufs)
    if (kv.second.ptr) (void)hipFree(kv.second.ptr);
  for (auto& p : ws->plans) (void)hipfftDestroy(p.h);
  if (ws->pinned) (void)hipHostFree(ws->pinned);
  for (auto& kv : ws->tables) {
    if (kv.second.staging) (void)hipHostFree(kv.second.staging);
    if (kv.second.uploaded) (void)hipEventDestroy(kv.second.uploaded);
  }
  if (ws->side) {
    (void)hipStreamSynchronize(ws->side);
    (void)hipStreamDestroy(ws->side);
  }
  if (ws->ev_fork) (void)hipEventDestroy(ws->ev_fork);
  if (ws->ev_join) (void)hipEventDestroy(ws->ev_join);
  for (hipStream_t ps : {ws->plan_stream, ws->plan_stream1})
    if (ps) {
      (void)hipStreamSynchronize(ps);
      (void)hipStreamDestroy(ps);
    }
  for (hipEvent_t e : ws->ev_done)
    if (e) (void)hipEventDestroy(e);
  if (ws->ev_planned) (void)hipEventDestroy(ws->ev_planned);
  if (ws->ev_entry) (void)hipEventDestroy(ws->ev_entry);
  const int dev = ws->device;
  delete ws;
  if (prev_dev >= 0 && prev_dev != dev) (void)hipSetDevice(prev_dev);
}

// Frees the calling thread's workspaces (every device) when the thread ends.
struct WorkspaceReaper {
  bool armed = false;
  ~WorkspaceReaper() {
    if (!armed || std::this_thread::get_id() == g_load_thread) return;
    std::vector<Workspace*> mine;
    {
      std::lock_guard<std::mutex> lock(g_ws_mutex);
      for (auto it = g_ws.begin(); it != g_ws.end();) {
        if (it->first.second == std::this_thread::get_id()) {
          mine.push_back(it->second);
          it = g_ws.erase(it);
        } else {
          ++it;
        }
      }
    }
    for (Workspace* ws : mine) destroy_workspace(ws);
  }
};
static thread_local WorkspaceReaper g_reaper;

static Workspace* workspace() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const auto key = std::make_pair(dev, std::this_thread::get_id());
  g_reaper.armed = true;
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  auto it = g_ws.find(key);
  if (it != g_ws.end()) {
    ++it->second->call_seq;  // every entry point takes its workspace once per call
    return it->second;
  }
  Workspace* ws = new Workspace();
  ws->device = dev;
  g_ws[key] = ws;
  return ws;
}

// grow-only device buffer; returns nullptr (and sets the error) on failure
void* buf_bytes(Workspace* ws, const char* name, size_t bytes) {
  DevBuf& b = ws->bufs[(ws->parity_scope && ws->parity) ? std::string(name) + "~1" : std::string(name)];
  if (b.bytes < bytes) {
    if (b.ptr && b.ptr == (void*)ws->grid_clean) ws->grid_clean = nullptr;  // a new buffer is not known zero
    if (b.ptr) ws->saved_valid = false;  // the saved plan may point into it
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.bytes = 0;
    // 12.5 % headroom so slowly growing inputs do not reallocate every call
    const size_t want = bytes + bytes / 8;
    if (hipMalloc(&b.ptr, want) != hipSuccess) {
      (void)hipGetLastError();
      set_error(CIP_ENOMEM, std::string("hipMalloc failed for workspace buffer ") + name);
      return nullptr;
    }
    b.bytes = want;
  }
  return b.ptr;
}

// grow-only pinned host memory (the readback staging and each table's own)
static void* pinned_grow(void** p, size_t* have, size_t bytes) {
  if (*have < bytes) {
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipHostMalloc(p, bytes) != hipSuccess) {
      *p = nullptr;
      set_error(CIP_ENOMEM, "hipHostMalloc failed");
      return nullptr;
    }
    *have = bytes;
  }
  return *p;
}

void* pinned(Workspace* ws, size_t bytes) { return pinned_grow(&ws->pinned, &ws->pinned_bytes, bytes); }

int readback_bytes(Workspace* ws, hipStream_t s, std::initializer_list<DevSrc> src, void** host) {
  const auto slot = [](size_t bytes) { return (bytes + 7) & ~(size_t)7; };
  size_t total = 0;
  for (const DevSrc& c : src) total += slot(c.bytes);
  char* h = (char*)pinned(ws, total);
  if (!h) return CIP_ENOMEM;
  size_t at = 0;
  for (const DevSrc& c : src) {
    if (c.dev) CIP_HIP_CHECK(hipMemcpyAsync(h + at, c.dev, c.bytes, hipMemcpyDeviceToHost, s));
    at += slot(c.bytes);
  }
  CIP_HIP_CHECK(hipStreamSynchronize(s));
  *host = h;
  return CIP_OK;
}

int host_table_open(Workspace* ws, const char* name, const std::vector<double>& key, size_t bytes, void** staging) {
  HostTable& t = ws->tables[name];
  *staging = nullptr;
  if (t.key == key) return CIP_OK;
  t.key.clear();
  if (!t.uploaded) {
    CIP_HIP_CHECK(hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
  } else {
    // the last upload has read the staging (it has, unless that stream is far behind)
    CIP_HIP_CHECK(hipEventSynchronize(t.uploaded));
  }
  if (!pinned_grow(&t.staging, &t.staging_bytes, bytes)) return CIP_ENOMEM;
  *staging = t.staging;
  return CIP_OK;
}

int host_table_upload(Workspace* ws, const char* name, const std::vector<double>& key, void* dev, size_t bytes,
                      hipStream_t s) {
  HostTable& t = ws->tables[name];
  CIP_HIP_CHECK(hipMemcpyAsync(dev, t.staging, bytes, hipMemcpyHostToDevice, s));
  CIP_HIP_CHECK(hipEventRecord(t.uploaded, s));
  t.key = key;
  return CIP_OK;
}

int fft_plan(Workspace* ws, int64_t nu, int64_t nv, hipStream_t s, hipfftHandle* out) {
  for (auto& p : ws->plans)
    if (p.nu == nu && p.nv == nv) {
      if (hipfftSetStream(p.h, s) != HIPFFT_SUCCESS) return set_error(CIP_EHIP, "hipfftSetStream failed");
      *out = p.h;
      return CIP_OK;
    }
  hipfftHandle h;
  if (hipfftPlan2d(&h, (int)nu, (int)nv, HIPFFT_Z2Z) != HIPFFT_SUCCESS)
    return set_error(CIP_EHIP, "hipfftPlan2d failed");
  if (hipfftSetStream(h, s) != HIPFFT_SUCCESS) return set_error(CIP_EHIP, "hipfftSetStream failed");
  ws->plans.push_back({h, nu, nv});
  *out = h;
  return CIP_OK;
}

// exp(+2 pi i m / n), m < n, for the pruned FFT passes (cached per length)
int fft_twiddles(Workspace* ws, int64_t n, hipStream_t s, double** out) {
  const std::string name = "fft_twiddle_" + std::to_string(n);
  double* tw = buf<double>(ws, name.c_str(), 2 * n);
  if (!tw) return CIP_ENOMEM;
  *out = tw;
  return host_table(ws, name.c_str(), {(double)n}, tw, sizeof(double) * 2 * n, s, [n](void* staging) {
    double* h = (double*)staging;
    for (int64_t m = 0; m < n; ++m) {
      // long double arguments: each entry correctly rounded (to within an ulp)
      const long double a = 2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)n;
      h[2 * m] = (double)cosl(a);
      h[2 * m + 1] = (double)sinl(a);
    }
  });
}

int begin_call(void* hip_stream, bool profiled, Call* c) {
  g_last_error.clear();
  c->s = (hipStream_t)hip_stream;
  c->ws = workspace();
  if (!c->ws) return set_error(CIP_EHIP, "no HIP device");
  if (const int sr = settle_async(c->ws, c->s); sr != CIP_OK) return sr;
  c->profiled = profiled;
  if (profiled) {
    g_prof.reset();
    c->t0 = g_prof.mark(c->s);
  }
  return CIP_OK;
}

int end_call(const Call& c) {
  if (c.profiled) g_prof.span(5, c.t0, g_prof.mark(c.s));
  CIP_HIP_CHECK(hipStreamSynchronize(c.s));
  if (c.profiled) g_prof.finish();
  return CIP_OK;
}

void leave_queued(const Call& c) { c.ws->async_stream = c.s; }

}  // namespace cip

using namespace cip;

extern "C" {

const char* cip_last_error(void) { return g_last_error.c_str(); }

const char* cip_build_info(void) { return "libcip_hip gfx950 (CDNA4) v0.1.0"; }

int cip_profile_enable(int on) {
  g_prof.on = (on != 0);
  return CIP_OK;
}

int cip_profile_last(double* ms, int64_t* counts) {
  if (ms)
    for (int i = 0; i < CIP_PROFILE_PHASES; ++i) ms[i] = g_prof.ms[i];
  if (counts)
    for (int i = 0; i < CIP_PROFILE_COUNTS; ++i) counts[i] = g_prof.counts[i];
  return CIP_OK;
}

int cip_release_workspace(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(CIP_EHIP, "no HIP device");
  std::lock_guard<std::mutex> lock(g_ws_mutex);
  auto it = g_ws.find(std::make_pair(dev, std::this_thread::get_id()));
  if (it == g_ws.end()) return CIP_OK;
  Workspace* ws = it->second;
  g_ws.erase(it);
  destroy_workspace(ws);
  return CIP_OK;
}

}  // extern "C"

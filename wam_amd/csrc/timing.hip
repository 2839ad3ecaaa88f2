// Live per-launch timing (see timing.hpp): the WamTimer every launcher brackets its kernel with,
// and the wam_timing_* entry points that switch it on and drain the records.
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "timing.hpp"

namespace {
struct TimingRec {
  const char* name;
  hipEvent_t s, e;
  double bytes;
};
std::atomic<int> g_timing{0};
std::mutex g_timing_mu;
std::vector<TimingRec> g_timing_recs;
}  // namespace

WamTimer::WamTimer(hipStream_t st_, const char* name_, double bytes_) : st(st_), name(name_), bytes(bytes_) {
  if (!g_timing.load(std::memory_order_relaxed)) return;
  if (hipEventCreate(&s) != hipSuccess || hipEventCreate(&e) != hipSuccess) {
    s = e = nullptr;
    return;
  }
  (void)hipEventRecord(s, st);
}

WamTimer::~WamTimer() {
  if (!s) return;
  (void)hipEventRecord(e, st);
  std::lock_guard<std::mutex> lk(g_timing_mu);
  g_timing_recs.push_back({name, s, e, bytes});
}

extern "C" {

int wam_timing_enable(int on) {
  g_timing.store(on ? 1 : 0);
  return WAM_OK;
}

int wam_timing_drain(int max_records, char* names, float* ms, double* bytes) {
  if (max_records < 0 || (max_records > 0 && (!names || !ms || !bytes))) return -WAM_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(g_timing_mu);
  int n = 0;
  for (auto& r : g_timing_recs) {
    if (n < max_records) {
      float t = 0.f;
      if (hipEventSynchronize(r.e) == hipSuccess) (void)hipEventElapsedTime(&t, r.s, r.e);
      strncpy(names + 64 * n, r.name, 63);
      names[64 * n + 63] = 0;
      ms[n] = t;
      bytes[n] = r.bytes;
      ++n;
    }
    (void)hipEventDestroy(r.s);
    (void)hipEventDestroy(r.e);
  }
  g_timing_recs.clear();
  return n;
}

}  // extern "C"

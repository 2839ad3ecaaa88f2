// Sanitizer driver for the host side of libwam_hip.so (no reference counterpart):
// host-only plans (wam_plan_create_host) over odd, tiny, huge and invalid shapes, every level
// count, filter length and mode, then every host query the library answers from a plan -- band
// layout, reconstruction shape, workspace sizes, kernel capability checks and the kernel routes
// (which run the fused kernels' geometry / LDS / ring predicates) and the split-sigma workspace
// size -- with invariants checked, and the routes of the benchmark and edge plans pinned. It prints
// a digest of every plan's caps and workspace sizes, to compare two builds of the library. Built by
// tests/native/build_sanitized.sh with AddressSanitizer and UndefinedBehaviorSanitizer on the host
// code only (no GPU needed; compute entry points must refuse host plans).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/wam_hip.h"

static int fails = 0, made = 0, with_caps = 0;
// 64-bit FNV-1a over the caps and workspace sizes of every created plan: printed, never asserted
// (a kernel change may move it), so two builds can be compared for dispatch-relevant equivalence
static uint64_t digest = 0xcbf29ce484222325ull;
static void digest_i64(int64_t v) {
  for (int i = 0; i < 8; ++i) {
    digest ^= (uint64_t)(v >> (8 * i)) & 0xff;
    digest *= 0x100000001b3ull;
  }
}
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "check failed line %d: %s\n", __LINE__, #c); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// wam_plan_describe, parsed: "whole|level,level,..." per transform, the maps route and the caps
struct Routes {
  std::string ana, adj, syn, maps;
  int caps = -1;
  bool ok = false;
};

static bool one_of(const std::string& s, std::initializer_list<const char*> names) {
  for (const char* n : names)
    if (s == n) return true;
  return false;
}

// "whole|l0,l1,...": a known whole-transform route and exactly `levels` known level routes
static bool field_ok(const std::string& f, int levels, bool syn) {
  const size_t bar = f.find('|');
  if (bar == std::string::npos || !one_of(f.substr(0, bar), {"none", "plane", "tile1", "haar3"})) return false;
  int n = 0;
  for (size_t at = bar + 1; at <= f.size(); ++n) {
    size_t end = f.find(',', at);
    if (end == std::string::npos) end = f.size();
    const std::string lv = f.substr(at, end - at);
    if (!(syn ? one_of(lv, {"colstrip", "tile3", "axis"}) : one_of(lv, {"rows", "colstrip", "tile3", "axis"})))
      return false;
    at = end + 1;
  }
  return n == levels;
}

static Routes describe(const wam_plan* p, int levels) {
  Routes r;
  char buf[512], ana[200], adj[200], syn[32], maps[16];
  CHECK(wam_plan_describe(p, buf, 8) == WAM_ERR_INVALID_ARG);  // too small: refused, not truncated
  CHECK(wam_plan_describe(p, nullptr, 512) == WAM_ERR_INVALID_ARG);
  if (wam_plan_describe(p, buf, (int)sizeof(buf)) != WAM_OK) return r;
  if (std::sscanf(buf, "ana=%199s adj=%199s syn=%31s maps=%15s caps=%d", ana, adj, syn, maps, &r.caps) != 5) return r;
  r.ana = ana, r.adj = adj, r.syn = syn, r.maps = maps;
  r.ok = field_ok(r.ana, levels, false) && field_ok(r.adj, levels, false) && field_ok(r.syn, 1, true) &&
         one_of(r.maps, {"none", "plane", "rows"});
  return r;
}

static std::string times(const char* whole, const char* level, int levels) {
  std::string s = std::string(whole) + "|";
  for (int l = 0; l < levels; ++l) s += std::string(l ? "," : "") + level;
  return s;
}

static void probe(int ndim, const int64_t* shape, int levels, int L, int mode, int flags) {
  std::vector<double> f(L > 0 ? L : 1, 0.25);
  wam_plan* p = nullptr;
  const int rc = wam_plan_create_host(&p, ndim, shape, levels, f.data(), f.data(), f.data(), f.data(), L, mode, flags);
  if (rc != WAM_OK) {
    CHECK(p == nullptr);
    CHECK(wam_strerror(rc) != nullptr);
    return;
  }
  ++made;
  const int nb = wam_plan_num_bands(p);
  CHECK(nb == 1 + levels * ((1 << ndim) - 1));
  int64_t prev = -1, dims[3];
  for (int b = 0; b < nb; ++b) {
    const int64_t off = wam_plan_band_offset(p, b);
    CHECK(off > prev);
    prev = off;
    CHECK(wam_plan_band_shape(p, b, dims) == WAM_OK);
    for (int a = 0; a < ndim; ++a) CHECK(dims[a] >= 1);
  }
  CHECK(wam_plan_band_shape(p, nb, dims) != WAM_OK);   // out of range
  CHECK(wam_plan_band_shape(p, -1, dims) != WAM_OK);
  CHECK(wam_plan_coeff_numel(p) > prev);
  CHECK(wam_plan_rec_shape(p, dims) == WAM_OK);
  for (int a = 0; a < ndim; ++a) CHECK(dims[a] >= shape[a] && dims[a] <= shape[a] + 1);
  const int caps = wam_plan_caps(p);  // the fused kernels' support predicates
  digest_i64(caps);
  for (int64_t batch : {int64_t(0), int64_t(1), int64_t(7), int64_t(4800)}) {
    const int64_t ws = wam_plan_workspace_bytes(p, batch);
    CHECK(ws >= 0);
    digest_i64(ws);
  }
  CHECK((caps & ~(WAM_CAP_NOISY_WAVEDEC | WAM_CAP_ADJOINT_MAPS | WAM_CAP_BF16_NHWC)) == 0);
  // the bf16 hand-off needs the fused maps pass
  CHECK(!(caps & WAM_CAP_BF16_NHWC) || (caps & WAM_CAP_ADJOINT_MAPS));
  with_caps += caps != 0;
  // the kernel routes: the line parses, agrees with the caps, and the flags narrow it as documented
  const Routes r = describe(p, levels);
  CHECK(r.ok);
  CHECK(r.caps == caps);
  CHECK(((caps & WAM_CAP_ADJOINT_MAPS) != 0) == (r.maps != "none"));
  if (caps & WAM_CAP_BF16_NHWC) CHECK(r.syn.rfind("plane|", 0) == 0 && r.maps == "plane");
  if (flags & WAM_PLAN_GENERIC) {
    CHECK(r.ana == times("none", "axis", levels) && r.adj == r.ana);
    CHECK(r.syn == "none|axis" && r.maps == "none" && caps == 0);
  }
  // compute entry points refuse a host-only plan before touching any buffer
  float dummy[4] = {0, 0, 0, 0};
  CHECK(wam_wavedec(p, 1, dummy, dummy, dummy, nullptr) == WAM_ERR_INVALID_ARG);
  CHECK(wam_waverec_bf16_nhwc(p, 3, dummy, nullptr, 1, 3, dummy, nullptr) == WAM_ERR_INVALID_ARG);
  CHECK(wam_waverec_adjoint_maps_bf16_nhwc(p, 1, 1, 3, dummy, dummy, dummy, nullptr) == WAM_ERR_INVALID_ARG);
  CHECK(wam_waverec(p, 1, dummy, nullptr, 1, dummy, dummy, nullptr) == WAM_ERR_INVALID_ARG);
  CHECK(wam_waverec_adjoint(p, 1, dummy, dummy, dummy, nullptr) == WAM_ERR_INVALID_ARG);
  wam_plan_destroy(p);
}

// the routes of one plan, pinned (filter values do not enter the routes: probe()'s constant taps)
static void golden(int ndim, std::initializer_list<int64_t> shape, int levels, int L, int mode, int flags,
                   const std::string& ana, const std::string& adj, const char* syn, const char* maps, int caps) {
  std::vector<double> f(L, 0.25);
  wam_plan* p = nullptr;
  CHECK(wam_plan_create_host(&p, ndim, shape.begin(), levels, f.data(), f.data(), f.data(), f.data(), L, mode, flags) ==
        WAM_OK);
  if (!p) return;
  const Routes r = describe(p, levels);
  if (!(r.ok && r.ana == ana && r.adj == adj && r.syn == syn && r.maps == maps && r.caps == caps)) {
    std::fprintf(stderr, "golden ndim %d L %d levels %d flags %d: ana=%s adj=%s syn=%s maps=%s caps=%d\n", ndim, L,
                 levels, flags, r.ana.c_str(), r.adj.c_str(), r.syn.c_str(), r.maps.c_str(), r.caps);
    ++fails;
  }
  wam_plan_destroy(p);
}

static void goldens() {
  const int G = WAM_PLAN_GENERIC;
  // 2D db4 and haar 224^2 J=3 reflect (c1 / c2): plane everywhere, the bf16 hand-off
  for (int L : {8, 2}) {
    golden(2, {224, 224}, 3, L, WAM_MODE_REFLECT, 0, times("plane", "rows", 3), times("plane", "rows", 3),
           "plane|colstrip", "plane", 7);
    golden(2, {224, 224}, 3, L, WAM_MODE_REFLECT, G, times("none", "axis", 3), times("none", "axis", 3), "none|axis",
           "none", 0);
  }
  golden(2, {224, 224}, 3, 8, WAM_MODE_REFLECT, WAM_PLAN_NO_PLANE, times("none", "rows", 3), times("none", "rows", 3),
         "none|colstrip", "rows", 3);
  golden(2, {224, 224}, 3, 8, WAM_MODE_REFLECT, WAM_PLAN_NO_ROWS, times("none", "colstrip", 3),
         times("none", "colstrip", 3), "none|colstrip", "none", 0);
  // 2D sym8 512^2 J=5 reflect (c4): rows too wide and the filter too long for the plane kernels
  golden(2, {512, 512}, 5, 16, WAM_MODE_REFLECT, 0, times("none", "rows", 5), times("none", "rows", 5), "none|colstrip",
         "rows", 3);
  golden(2, {512, 512}, 5, 16, WAM_MODE_REFLECT, G, times("none", "axis", 5), times("none", "axis", 5), "none|axis",
         "none", 0);
  // 2D db3 226^2 J=3 zero: a width that is no multiple of 4 keeps the analyses off the plane kernel
  // and the noise off level 0; the synthesis still runs plane-resident
  golden(2, {226, 226}, 3, 6, WAM_MODE_ZERO, 0, times("none", "rows", 3), times("none", "rows", 3), "plane|colstrip",
         "rows", 2);
  golden(2, {226, 226}, 3, 6, WAM_MODE_ZERO, G, times("none", "axis", 3), times("none", "axis", 3), "none|axis", "none",
         0);
  // 2D db5 (10 taps: no row or plane instantiation) 64 x 96 J=2 reflect
  golden(2, {64, 96}, 2, 10, WAM_MODE_REFLECT, 0, times("none", "colstrip", 2), times("none", "colstrip", 2),
         "none|colstrip", "none", 0);
  golden(2, {64, 96}, 2, 10, WAM_MODE_REFLECT, G, times("none", "axis", 2), times("none", "axis", 2), "none|axis",
         "none", 0);
  // 1D db6 80,000 J=5 reflect (c3)
  golden(1, {80000}, 5, 12, WAM_MODE_REFLECT, 0, times("tile1", "axis", 5), times("tile1", "axis", 5), "tile1|axis",
         "none", 1);
  golden(1, {80000}, 5, 12, WAM_MODE_REFLECT, G, times("none", "axis", 5), times("none", "axis", 5), "none|axis", "none",
         0);
  // 3D haar 128^3 J=2 symmetric (c5), and db2 at odd sizes
  golden(3, {128, 128, 128}, 2, 2, WAM_MODE_SYMMETRIC, 0, times("haar3", "tile3", 2), times("haar3", "tile3", 2),
         "haar3|tile3", "none", 1);
  golden(3, {128, 128, 128}, 2, 2, WAM_MODE_SYMMETRIC, G, times("none", "axis", 2), times("none", "axis", 2),
         "none|axis", "none", 0);
  golden(3, {33, 20, 17}, 2, 4, WAM_MODE_SYMMETRIC, 0, times("none", "tile3", 2), times("none", "tile3", 2),
         "none|tile3", "none", 0);
  golden(3, {33, 20, 17}, 2, 4, WAM_MODE_SYMMETRIC, G, times("none", "axis", 2), times("none", "axis", 2), "none|axis",
         "none", 0);
}

int main() {
  const int Ls[] = {2, 4, 6, 8, 10, 12, 16, 20, 40, 128, 0, 3, 130};
  const int64_t edge[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 33, 63, 64, 65, 127, 224, 255, 256, 257, 511, 512, 513,
                          4095, 80000, 1 << 20, int64_t(1) << 30, (int64_t(1) << 31) - 1, int64_t(1) << 31,
                          int64_t(1) << 40, -1, 0};
  const int ne = sizeof(edge) / sizeof(edge[0]);
  int n = 0;
  for (int ndim = 0; ndim <= 4; ++ndim)
    for (int levels : {0, 1, 2, 3, 5, 8, 16, 17})
      for (int L : Ls)
        for (int mode = -1; mode <= 5; ++mode)
          for (int k = 0; k < 6; ++k) {
            int64_t shape[3];
            for (int a = 0; a < 3; ++a) shape[a] = (k < 2) ? edge[(k * 7 + a * 3 + levels) % ne] : edge[rnd() % ne];
            const int flags = (int)(rnd() % 64);
            probe(ndim, shape, levels, L, mode, flags);
            ++n;
          }
  // the benchmark configurations (c1/c2 224^2, c4 512^2 sym8 J=5, c3 80,000-sample db6 J=5, c5 128^3
  // haar J=2) under every flag combination: the fused kernels' predicates on real geometries
  const int64_t s224[2] = {224, 224}, s512[2] = {512, 512}, s1[1] = {80000}, s3[3] = {128, 128, 128};
  for (int fl = 0; fl < 64; ++fl)
    for (int mode = 0; mode <= 4; ++mode) {
      probe(2, s224, 3, 8, mode, fl);
      probe(2, s224, 3, 2, mode, fl);
      probe(2, s512, 5, 16, mode, fl);
      probe(1, s1, 5, 12, mode, fl);
      probe(3, s3, 2, 2, mode, fl);
    }
  goldens();
  // null / invalid arguments
  {
    char buf[8];
    CHECK(wam_plan_describe(nullptr, buf, 8) == WAM_ERR_INVALID_ARG);
  }
  CHECK(wam_plan_create_host(nullptr, 2, nullptr, 1, nullptr, nullptr, nullptr, nullptr, 2, 0, 0) != WAM_OK);
  CHECK(wam_plan_num_bands(nullptr) < 0);
  CHECK(wam_plan_caps(nullptr) == 0);
  CHECK(wam_item_sigma_ws_bytes(0, 5) == 0);
  CHECK(wam_item_sigma_ws_bytes(64, 150528) > 0);
  CHECK(wam_item_sigma_ws_bytes(1, int64_t(1) << 40) > 0);
  // .scales of a map smaller than 2^levels: an empty coarsest quadrant, refused before any launch
  // (the pointers are never used)
  {
    double avg[36] = {0}, out[4 * 36] = {0};
    const int small[3][2] = {{4, 3}, {6, 3}, {3, 2}};
    for (const auto& c : small)
      for (int approx = 0; approx <= 1; ++approx)
        CHECK(wam_reproject_scales(1, c[0], c[1], approx, avg, out, nullptr) == WAM_ERR_INVALID_ARG);
  }
  std::printf("plan_fuzz: %d random plans probed, %d plans created, %d with fused-kernel caps, %d failed checks\n",
              n, made, with_caps, fails);
  std::printf("plan_fuzz: caps/workspace digest %016llx\n", (unsigned long long)digest);
  return fails ? 1 : 0;
}

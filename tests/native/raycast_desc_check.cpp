// raycast_desc_check.cpp -- CPU check of maniskill_amd/csrc/mssim_raycast_desc.h: what mssim_raycast_create accepts. A
// valid scene with every table exactly as long as its counts say (so that a read past an end is an AddressSanitizer
// report), then one defect at a time: each is refused with its return code and a message, and nothing else changes the
// verdict. Stand-alone (tests/test_raycast.py builds it with ASan + UBSan and expects exit status 0).
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../maniskill_amd/csrc/mssim_raycast_desc.h"

static int g_failed = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond);   \
      g_failed++;                                                            \
    }                                                                        \
  } while (0)

namespace {

constexpr int N = 3, ROWS = 4;

// a scene on the heap: 4 shapes (plane, box with a per-env slot, convex with 5 planes, sphere), 1 override slot
struct Scene {
  std::vector<int32_t> type{MSSIM_SHAPE_PLANE, MSSIM_SHAPE_BOX, MSSIM_SHAPE_CONVEX, MSSIM_SHAPE_SPHERE};
  std::vector<int32_t> row{-1, 0, 3, 2};
  std::vector<float> frame, param, bound;
  std::vector<int16_t> seg{1, 2, 3, 4};
  std::vector<int32_t> planes2{0, 0, 0, 0, 1, 5, 0, 0};
  std::vector<float> planes;
  std::vector<int32_t> slot{-1, 0, -1, -1};
  std::vector<float> env_frame, env_param, env_bound;
  mssim_raycast_scene d{};
  Scene() {
    for (int i = 0; i < 4; i++) {
      const float f[7] = {0.1f * i, 0, 0, 1, 0, 0, 0};
      frame.insert(frame.end(), f, f + 7);
      const float p[4] = {0.1f, 0.2f, 0.3f, 0};
      param.insert(param.end(), p, p + 4);
      const float b[4] = {0, 0, 0, i == 0 ? -1.f : 0.5f};
      bound.insert(bound.end(), b, b + 4);
    }
    for (int k = 0; k < 6; k++) {
      const float pl[4] = {k == 0 ? 1.f : 0.f, k == 1 ? 1.f : 0.f, k >= 2 ? 1.f : 0.f, 0.1f};
      planes.insert(planes.end(), pl, pl + 4);
    }
    env_frame.assign(7 * N, 0.f);
    for (int e = 0; e < N; e++) env_frame[3 * N + e] = 1.f;
    env_param.assign(4 * N, 0.05f);
    const float types[N] = {0.f, (float)(MSSIM_SHAPE_SPHERE + 1), (float)(MSSIM_SHAPE_NONE + 1)};
    for (int e = 0; e < N; e++) env_param[3 * N + e] = types[e];
    env_bound.assign(4 * N, 0.1f);
    link();
  }
  void link() {
    d.n_shape = (int32_t)type.size();
    d.shape_type = type.data(); d.shape_row = row.data(); d.shape_frame = frame.data(); d.shape_param = param.data();
    d.shape_bound = bound.data(); d.shape_seg = seg.data(); d.shape_planes = planes2.data();
    d.n_plane = (int32_t)planes.size() / 4; d.planes = planes.data();
    d.n_env_shape = 1; d.shape_env_slot = slot.data();
    d.env_shape_frame = env_frame.data(); d.env_shape_param = env_param.data(); d.env_shape_bound = env_bound.data();
  }
};

mssim_camera_desc good_camera() {
  mssim_camera_desc c{};
  c.width = 32; c.height = 24; c.fx = c.fy = 20.f; c.cx = 16.f; c.cy = 12.f; c.near = 0.01f; c.far = 100.f; c.mount_row = -1;
  c.pose[3] = 1.f;
  return c;
}

int verdict(const Scene& s, const std::vector<mssim_camera_desc>& cams, std::string* err, int n_envs = N) {
  return mssim_raycast::validate(&s.d, cams.data(), (int)cams.size(), n_envs, ROWS, err);
}

// the defect is refused with `rc`, and the message names `word`
template <class Break>
void refused(int rc, const char* word, Break brk) {
  Scene s;
  std::vector<mssim_camera_desc> cams{good_camera()};
  brk(s, cams);
  s.link();
  std::string err;
  const int got = verdict(s, cams, &err);
  if (got != rc || err.find(word) == std::string::npos) std::printf("expected rc %d with '%s', got rc %d: %s\n", rc, word, got, err.c_str());
  CHECK(got == rc);
  CHECK(err.find("raycast_create: ") == 0);
  CHECK(err.find(word) != std::string::npos);
}

}  // namespace

int main() {
  {
    Scene s;
    std::vector<mssim_camera_desc> cams{good_camera(), good_camera()};
    cams[1].width = 1; cams[1].height = 1; cams[1].mount_row = ROWS - 1;
    std::string err = "untouched";
    CHECK(verdict(s, cams, &err) == 0);
    CHECK(err == "untouched");
    CHECK(mssim_raycast::validate(&s.d, cams.data(), 2, N, ROWS, nullptr) == 0);  // (no message wanted)
    // an empty scene is a scene
    mssim_raycast_scene empty{};
    CHECK(mssim_raycast::validate(&empty, cams.data(), 1, N, ROWS, &err) == 0);
  }
  using Cams = std::vector<mssim_camera_desc>;
  refused(3, "triangle mesh", [](Scene& s, Cams&) { s.type[3] = MSSIM_SHAPE_TRIMESH; });
  refused(3, "triangle mesh", [](Scene& s, Cams&) { s.env_param[3 * N + 1] = (float)(MSSIM_SHAPE_TRIMESH + 1); });
  refused(3, "per-env hulls", [](Scene& s, Cams&) { s.env_param[3 * N + 2] = (float)(MSSIM_SHAPE_CONVEX + 1); });
  refused(2, "body row", [](Scene& s, Cams&) { s.row[1] = ROWS; });
  refused(2, "body row", [](Scene& s, Cams&) { s.row[0] = -2; });
  refused(2, "plane range", [](Scene& s, Cams&) { s.planes2[5] = 6; });   // one past the table
  refused(2, "plane range", [](Scene& s, Cams&) { s.planes2[4] = -1; });
  refused(2, "plane range", [](Scene& s, Cams&) { s.planes2[5] = 3; });   // fewer than a tetrahedron's
  refused(2, "override slot", [](Scene& s, Cams&) { s.slot[3] = 1; });
  refused(2, "per-env type", [](Scene& s, Cams&) { s.env_param[3 * N] = 9.f; });
  refused(2, "per-env type", [](Scene& s, Cams&) { s.env_param[3 * N] = 1.5f; });
  refused(2, "unknown type", [](Scene& s, Cams&) { s.type[0] = 8; });
  refused(1, "plane cannot be a per-env shape", [](Scene& s, Cams&) { s.slot[0] = 0; });
  refused(1, "not finite", [](Scene& s, Cams&) { s.frame[8] = std::numeric_limits<float>::infinity(); });
  refused(1, "not finite", [](Scene& s, Cams&) { s.env_bound[N] = std::numeric_limits<float>::quiet_NaN(); });
  refused(4, "image size", [](Scene&, Cams& c) { c[0].width = 0; });
  refused(4, "image size", [](Scene&, Cams& c) { c[0].height = 5000; });
  refused(4, "near", [](Scene&, Cams& c) { c[0].near = 0.f; });
  refused(4, "near", [](Scene&, Cams& c) { c[0].far = 0.005f; });
  refused(4, "intrinsics", [](Scene&, Cams& c) { c[0].fx = 0.f; });
  refused(2, "mount row", [](Scene&, Cams& c) { c[0].mount_row = ROWS; });
  refused(4, "pose", [](Scene&, Cams& c) { c[0].pose[0] = std::numeric_limits<float>::quiet_NaN(); });
  {
    Scene s;
    std::vector<mssim_camera_desc> cams{good_camera()};
    std::string err;
    CHECK(mssim_raycast::validate(nullptr, cams.data(), 1, N, ROWS, &err) == 1);
    CHECK(mssim_raycast::validate(&s.d, nullptr, 1, N, ROWS, &err) == 1);
    CHECK(mssim_raycast::validate(&s.d, cams.data(), 0, N, ROWS, &err) == 1);
    CHECK(verdict(s, cams, &err, 0) == 1);
    s.d.shape_seg = nullptr;
    CHECK(verdict(s, cams, &err) == 1 && err.find("table is missing") != std::string::npos);
  }
  if (g_failed) {
    std::printf("raycast_desc_check: %d failed\n", g_failed);
    return 1;
  }
  std::printf("raycast_desc_check: ok\n");
  return 0;
}

// Host check of the producer's host half (csrc/svsdf_points.hpp), compiled for the host alone with the address and
// undefined-behaviour sanitizers: svsdf_host::path_waypoints, and GridGeometry::centre_boxes -- the index boxes the device
// gather takes from the host -- against OccupancyMap::gather, which walks the same boxes.
//   mapgeom_host bmin[3] bmax[3] resolution : prints the 12 ints per centre of the six test centres on that grid ("box ..."),
//   then runs the self-checks and prints "all checks passed"; exit code 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../implicit-svsdf-planner_amd/csrc/svsdf_points.hpp"

using svsdf_host::GridGeometry;
using svsdf_host::OccupancyMap;

static int bad = 0;
static void check(bool ok, const char *what) {
  if (!ok) { std::printf("MISMATCH %s\n", what); ++bad; }
}

int main(int argc, char **argv) {
  if (argc != 8) { std::printf("usage: mapgeom_host bmin[3] bmax[3] resolution\n"); return 2; }
  GridGeometry g;
  for (int d = 0; d < 3; ++d) { g.bmin_[d] = std::atof(argv[1 + d]); g.bmax_[d] = std::atof(argv[4 + d]); }
  g.set_resolution(std::atof(argv[7]));
  std::printf("dims %d %d %d cells %zu\n", g.size_[0], g.size_[1], g.size_[2], g.cells());
  const double ext[3] = {12.0, 20.0, 3.0}, fr[5] = {0.1, 0.3, 0.3, 0.55, 0.8};
  std::vector<double> centres;
  for (double f : fr) { centres.push_back(f * ext[0]); centres.push_back(f * ext[1]); centres.push_back(0.4); }
  centres.push_back(ext[0] + 5); centres.push_back(ext[1] + 5); centres.push_back(0.4);
  const double res = g.res_, halfbd[3] = {17 * res / 3, 17 * res / 3, 17 * res / 3};
  std::vector<int> boxes;
  g.centre_boxes(centres.data(), centres.size() / 3, halfbd, boxes);
  for (size_t c = 0; c < centres.size() / 3; ++c) {
    std::printf("box");
    for (int q = 0; q < 12; ++q) std::printf(" %d", boxes[12 * c + q]);
    std::printf("\n");
  }
  g.centre_boxes(centres.data(), 0, halfbd, boxes);
  check(boxes.empty(), "no centres, no boxes");

  // a map of 700 points on the same extent: the gather rebuilt from centre_boxes + cell() equals OccupancyMap::gather
  std::vector<float> cloud;
  unsigned long long s = 20240807ull;
  for (int i = 0; i < 700; ++i)
    for (int d = 0; d < 3; ++d) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      cloud.push_back((float)((double)(s >> 11) / 9007199254740992.0 * ext[d]));
    }
  OccupancyMap m;
  m.build(cloud.data(), cloud.size() / 3, 1.0, 1);
  GridGeometry h;
  for (int d = 0; d < 3; ++d) { h.bmin_[d] = m.bmin()[d]; h.bmax_[d] = m.bmax()[d]; }
  h.set_resolution(1.0);
  for (int d = 0; d < 3; ++d) check(h.size_[d] == m.dims()[d], "dims from the bounds");
  const double hb[3] = {17 / 3.0, 17 / 3.0, 17 / 3.0};
  std::vector<double> want, got;
  m.gather(centres.data(), centres.size() / 3, hb, want);
  h.centre_boxes(centres.data(), centres.size() / 3, hb, boxes);
  std::set<int> ids;
  for (size_t c = 0; c < centres.size() / 3; ++c) {
    const int *b = boxes.data() + 12 * c;
    for (int i = b[0]; i <= b[3]; ++i)
      for (int j = b[1]; j <= b[4]; ++j)
        for (int k = b[2]; k <= b[5]; ++k)
          if ((i > b[9] || i < b[6] || j > b[10] || j < b[7] || k > b[11] || k < b[8]) && m.cell(i, j, k))
            ids.insert(k * h.size_[0] * h.size_[1] + j * h.size_[0] + i);
  }
  for (int uid : ids) {
    double p[3];
    h.cube_center(uid % h.size_[0], (uid / h.size_[0]) % h.size_[1], uid / (h.size_[0] * h.size_[1]), p);
    got.insert(got.end(), p, p + 3);
  }
  check(!want.empty() && got == want, "gather from centre_boxes");
  std::printf("gathered %zu\n", want.size() / 3);

  // the waypoint loop
  std::vector<size_t> idx;
  int gap = 0;
  check(svsdf_host::path_waypoints(70, 1.0, 3.0, idx, &gap) && gap == 3 && idx.size() == 22 && idx.front() == 3 && idx.back() == 66,
        "waypoints 70");
  check(svsdf_host::path_waypoints(3, 1.0, 3.0, idx, &gap) && gap == 1 && idx.size() == 1 && idx[0] == 1, "waypoints 3 (shrink)");
  check(svsdf_host::path_waypoints(10, 1e-300, 1e300, idx, &gap) && gap >= 1 && gap < 9, "waypoints: a quotient that overflows");
  check(!svsdf_host::path_waypoints(2, 1.0, 3.0, idx, &gap) && idx.empty(), "path_len 2 refused");
  check(!svsdf_host::path_waypoints(70, 0.0, 3.0, idx, &gap), "resolution 0 refused");
  check(!svsdf_host::path_waypoints(70, 1.0, -1.0, idx, &gap), "parlength < 0 refused");
  check(!svsdf_host::path_waypoints(70, 1.0, std::nan(""), idx, &gap), "NaN refused");
  if (bad) return 1;
  std::printf("all checks passed\n");
  return 0;
}

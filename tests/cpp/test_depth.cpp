// Depth images and point clouds through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_depth.h): the robot and
// spheres of tests/cpp/test_grid.cpp, a camera that looks along +x, two frames and a handful of points.  With a path as its argument the
// program writes the counters, the occupancy, the field and the clearance after every call there (raw doubles, the integers as doubles),
// for tests/test_cpp_depth.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cstddef>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_DEPTH_VERSION == 1, "the version of loik_amd_depth.h");
static_assert(LOIKB_DEPTH_F32 == 0 && LOIKB_DEPTH_U16 == 1 && LOIKB_DEPTH_REPLACE == 0 && LOIKB_DEPTH_FUSE == 1 && LOIKB_DEPTH_Q_DEVICE == 2, "the constants");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_depth_version() != LOIKB_DEPTH_VERSION) { ++failures; std::printf("loikb_depth_version() = %d\n", loikb_depth_version()); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec qa((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  std::vector<Index> links;
  DVec spheres;
  for (int l = 1; l <= 7; ++l)
    for (int k = 0; k < 2; ++k) {
      links.push_back(l);
      for (double v : {((l + k) % 5 - 2) / 64.0, ((2 * l + k) % 7 - 3) / 64.0, (k ? 4 : -3) / 64.0, (2 + (l + k) % 3) / 64.0}) spheres.push_back(v);
    }
  solver.setCollisionSpheres(links, spheres);

  FirstOrderLoikOptimized::DepthCamera cam;
  cam.width = 40; cam.height = 30;
  cam.fx = cam.fy = 32.0; cam.cx = 19.5; cam.cy = 14.5;
  cam.T_world_cam = {{0, 0, 1, -1, 0, 0, 0, -1, 0, -1.0, 0.0, 0.375}};
  cam.z_min = 0.25; cam.z_max = 8.0;
  const std::array<int, 3> dims{{19, 17, 15}};
  const std::array<double, 3> origin{{-0.5 + 1.0 / 8192, -0.53125 + 1.0 / 8192, -0.03125 + 1.0 / 8192}};
  const double voxel = 0.0625;
  std::vector<float> f1((std::size_t)cam.width * cam.height);
  std::vector<unsigned short> f2(f1.size());
  for (int v = 0; v < cam.height; ++v)
    for (int u = 0; u < cam.width; ++u) {
      const std::size_t i = (std::size_t)v * cam.width + u;
      f1[i] = (u * 7 + v * 5) % 29 == 0 ? 0.0f : (float)(0.625 + ((u * 7 + v * 5) % 23) / 32.0);
      f2[i] = (unsigned short)((u + v) % 31 == 0 ? 0 : 640 + 32 * ((u * 3 + v * 11) % 27));   // units of 1 / 1024 m
    }
  DVec all;
  auto record = [&](const FirstOrderLoikOptimized::DepthStats& st, const char* what) {
    std::vector<unsigned char> occ;
    FirstOrderLoikOptimized::CollisionGrid g;
    if (!solver.GetCollisionOccupancy(&occ) || !solver.GetCollisionGrid(&g) || occ.size() != g.G.size()) { ++failures; std::printf("%s: no grid\n", what); return; }
    long long n = 0;
    for (std::size_t i = 0; i < occ.size(); ++i) {
      n += occ[i];
      if (occ[i] > 1 || (occ[i] == 1) != (g.G[i] == 0u)) { ++failures; std::printf("%s: occupancy and field differ at %zu\n", what, i); break; }
    }
    if (n != st.occupied_after || st.inside > st.returns) { ++failures; std::printf("%s: the counters\n", what); }
    for (long long v : {st.returns, st.inside, st.occupied_before, st.occupied_after}) all.push_back((double)v);
    all.insert(all.end(), occ.begin(), occ.end());
    all.insert(all.end(), g.G.begin(), g.G.end());
    const auto clr = solver.Clearance();
    all.insert(all.end(), clr.min.begin(), clr.min.end());
  };
  if (solver.GetCollisionOccupancy()) { ++failures; std::printf("an occupancy before a grid\n"); }
  FirstOrderLoikOptimized::DepthOptions opt;
  opt.filter_resident = 2;
  opt.filter_pad = 0.0625;
  const auto s1 = solver.IntegrateDepth(f1, cam, dims, origin, voxel, opt);
  record(s1, "replace");
  if (s1.occupied_before != 0 || s1.inside == 0) { ++failures; std::printf("replace: the counters\n"); }
  cam.depth_scale = 1.0 / 1024;
  opt.fuse = opt.carve = true;   // the recommended band
  opt.filter_resident = 0;
  opt.filter_q.assign(qa.begin(), qa.begin() + 3 * model.nq);
  const auto s2 = solver.IntegrateDepth(f2, cam, dims, origin, voxel, opt);
  record(s2, "fuse");
  if (s2.occupied_before != s1.occupied_after) { ++failures; std::printf("fuse: the prior is not the grid that was set\n"); }
  DVec pts;
  for (int i = 0; i < 50; ++i)
    for (double v : {((i * 7) % 19 - 9) / 16.0 + 1.0 / 256, ((i * 5) % 17 - 8) / 16.0 + 1.0 / 512, ((i * 3) % 13) / 16.0 + 3.0 / 1024}) pts.push_back(v);
  FirstOrderLoikOptimized::DepthOptions popt;
  popt.fuse = true;
  popt.filter_pad = 0.0;
  popt.filter_resident = 1;
  const auto s3 = solver.IntegratePoints(pts, dims, origin, voxel, popt);
  record(s3, "points");
  if (s3.returns != 50 || s3.occupied_before != s2.occupied_after) { ++failures; std::printf("points: the counters\n"); }
  int n_threw = 0;
  popt.carve = true;
  try { solver.IntegratePoints(pts, dims, origin, voxel, popt); } catch (const std::runtime_error&) { ++n_threw; }
  opt.fuse = false;
  try { solver.IntegrateDepth(f1, cam, dims, origin, voxel, opt); } catch (const std::runtime_error&) { ++n_threw; }
  f1.pop_back();
  try { solver.IntegrateDepth(f1, cam, dims, origin, voxel); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 3) { ++failures; std::printf("%d of 3 bad calls threw\n", n_threw); }
  solver.ClearCollisionGrid();
  if (solver.GetCollisionOccupancy()) { ++failures; std::printf("an occupancy after the grid was cleared\n"); }
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all depth checks passed\n");
  return 0;
}

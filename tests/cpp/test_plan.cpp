// Planning through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_plan.h): Panda-7, two spheres per link, a
// world of two spheres and one box, self pairs; the configurations of tests/cpp/test_motion.cpp, query b from row b to row b + 16.  With a
// path as its argument the program writes what PlanPaths returned there (raw doubles, the integers as doubles), for
// tests/test_cpp_plan.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_PLAN_VERSION == 1, "the version of loik_amd_plan.h");
static_assert(sizeof(loikb_plan_params) == 48, "three doubles, a 64-bit seed, four ints: no padding");
static_assert(offsetof(loikb_plan_params, seed) == 24 && offsetof(loikb_plan_params, max_evals) == 32 && offsetof(loikb_plan_params, flags) == 44, "the layout");

static void append(DVec& all, const FirstOrderLoikOptimized::PlanResult& r)
{
  all.insert(all.end(), r.q_path.begin(), r.q_path.end());
  for (const std::vector<int>* v : {&r.n_waypoints, &r.status, &r.iterations, &r.nodes, &r.edges_checked, &r.edges_free, &r.evals}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), r.length.begin(), r.length.end());
}

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_plan_version() != LOIKB_PLAN_VERSION) { ++failures; std::printf("loikb_plan_version() = %d, header %d\n", loikb_plan_version(), LOIKB_PLAN_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67, Bq = 16, T = 16;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations that are the same doubles in any language: sixteenths
  DVec qa((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  const DVec q_start(qa.begin(), qa.begin() + (std::size_t)Bq * model.nq), q_goal(qa.begin() + (std::size_t)Bq * model.nq, qa.begin() + (std::size_t)2 * Bq * model.nq);
  const DVec s_lo(model.nv, -1.0), s_hi(model.nv, 1.0);
  bool threw = false;
  try { (void)solver.PlanPaths(q_start, q_goal, s_lo, s_hi, T); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("PlanPaths without spheres did not throw\n"); }
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
  solver.setCollisionWorld({0.25, 0.0, 0.5, 0.125, -0.5, 0.25, 0.25, 0.0625}, {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 0.0, -0.25, 1.0, 1.0, 0.125});
  solver.setSelfCollision(true, {{2, 4}});
  const double margin = -0.0625, tol = 1.0 / 1024, step = 0.5;
  const auto r = solver.PlanPaths(q_start, q_goal, s_lo, s_hi, T, step, 16, 32, 99ull, margin, tol, 64);
  const auto direct = solver.PlanPaths(q_start, q_goal, s_lo, s_hi, T, step, 0, 32, 99ull, margin, tol, 64);
  int found = 0;
  for (int b = 0; b < Bq; ++b) {
    const int L = r.n_waypoints[b];
    const double* path = r.q_path.data() + (std::size_t)b * T * model.nq;
    if (r.status[b] != LOIKB_PLAN_FOUND) {
      if (!std::isnan(path[0]) || !std::isnan(r.length[b])) { ++failures; std::printf("query %d: rows of a path that was not found\n", b); }
      continue;
    }
    ++found;
    if (L < 2 || L > T || !(r.length[b] > 0.0) || r.edges_free[b] > r.edges_checked[b]) { ++failures; std::printf("query %d: L, the length or the counters\n", b); continue; }
    for (int c = 0; c < model.nq; ++c) {
      if (path[c] != q_start[(std::size_t)b * model.nq + c]) { ++failures; std::printf("query %d: row 0\n", b); break; }
      if (path[(std::size_t)(L - 1) * model.nq + c] != q_goal[(std::size_t)b * model.nq + c] || path[(std::size_t)(T - 1) * model.nq + c] != q_goal[(std::size_t)b * model.nq + c]) { ++failures; std::printf("query %d: the last rows\n", b); break; }
    }
    if ((direct.status[b] == LOIKB_PLAN_FOUND) != (r.iterations[b] == 0)) { ++failures; std::printf("query %d: max_iters = 0\n", b); }
  }
  if (!found) { ++failures; std::printf("no path found\n"); }
  // every segment of a found path is FREE under the path check, and the length is PathLength's
  const auto chk = solver.PathClearance(r.q_path, T, margin, tol, 64);
  const DVec length = solver.PathLength(r.q_path, T);
  for (int b = 0; b < Bq; ++b) {
    if (r.status[b] != LOIKB_PLAN_FOUND) continue;
    for (int k = 0; k < T - 1; ++k)
      if (chk.status[(std::size_t)b * (T - 1) + k] != LOIKB_MOTION_FREE) { ++failures; std::printf("query %d: segment %d is not FREE\n", b, k); }
    if (length[b] != r.length[b]) { ++failures; std::printf("query %d: the length\n", b); }
  }
  // bad parameters are refused
  int n_threw = 0;
  try { (void)solver.PlanPaths(q_start, q_goal, s_lo, s_hi, T, 0.0); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.PlanPaths(q_start, q_goal, s_lo, s_hi, T, step, 16, 1); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.PlanPaths(q_start, q_goal, s_lo, s_hi, 1); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.PlanPaths(q_start, q_goal, s_hi, s_lo, T); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 4) { ++failures; std::printf("%d of 4 bad calls threw\n", n_threw); }
  DVec all;
  append(all, r);
  append(all, direct);
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all plan checks passed\n");
  return 0;
}

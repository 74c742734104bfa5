// The motion checks through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_motion.h): Panda-7, two spheres
// per link, a world of two spheres and one box, self pairs.  With a path as its argument the program writes what Difference,
// MotionClearance and PathClearance returned there (raw doubles, the integers as doubles), for tests/test_cpp_motion.py to compare with
// the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_MOTION_FREE == 0 && LOIKB_MOTION_BLOCKED == 1 && LOIKB_MOTION_UNDECIDED == 2 && LOIKB_MOTION_INVALID == 3, "the statuses of loik_amd_motion.h");
static_assert(sizeof(loikb_motion_params) == 24, "two doubles and two ints");

static void append(DVec& all, const FirstOrderLoikOptimized::MotionResult& r)
{
  all.insert(all.end(), r.status.begin(), r.status.end());
  all.insert(all.end(), r.evals.begin(), r.evals.end());
  all.insert(all.end(), r.s_free.begin(), r.s_free.end());
  all.insert(all.end(), r.min_sampled.begin(), r.min_sampled.end());
  all.insert(all.end(), r.s_at_min.begin(), r.s_at_min.end());
  all.insert(all.end(), r.witness.begin(), r.witness.end());
}

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_motion_version() != LOIKB_MOTION_VERSION) { ++failures; std::printf("loikb_motion_version() = %d, header %d\n", loikb_motion_version(), LOIKB_MOTION_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67, T = 4;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations and displacements that are the same doubles in any language: sixteenths and sixty-fourths
  DVec qa((std::size_t)B * model.nq), dv((std::size_t)B * model.nv);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) {
      qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
      dv[(std::size_t)b * model.nv + k] = ((b * 5 + 11 * k) % 23 - 11) / 64.0;
    }
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  bool threw = false;
  try { (void)solver.MotionClearance(qa, dv); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("MotionClearance without spheres did not throw\n"); }
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
  // the end points, and back: a plain difference on a revolute arm
  DVec qb(qa);
  for (std::size_t i = 0; i < qb.size(); ++i) qb[i] += dv[i];
  const DVec v = solver.Difference(qa, qb);
  if (v.size() != dv.size()) { ++failures; std::printf("Difference returned %zu values\n", v.size()); }
  for (std::size_t i = 0; i < v.size() && i < dv.size(); ++i)
    if (v[i] != qb[i] - qa[i]) { ++failures; std::printf("Difference: entry %zu\n", i); break; }
  const double margin = -0.0625, tol = 1.0 / 1024;
  const auto r = solver.MotionClearance(qa, dv, margin, tol, 16);
  const auto one = solver.MotionClearance(qa, dv, margin, tol, 1);
  int seen[4] = {0, 0, 0, 0};
  for (int b = 0; b < B; ++b) {
    const int st = r.status[b];
    if (st < LOIKB_MOTION_FREE || st > LOIKB_MOTION_UNDECIDED) { ++failures; std::printf("segment %d: status %d\n", b, st); continue; }
    ++seen[st];
    if (r.evals[b] < 1 || r.evals[b] > 16 || !(r.s_free[b] >= 0.0 && r.s_free[b] <= 1.0) || !(r.s_at_min[b] <= r.s_free[b])) { ++failures; std::printf("segment %d: evals / s\n", b); }
    if (st == LOIKB_MOTION_FREE && !(r.s_free[b] == 1.0 && r.min_sampled[b] >= margin + tol)) { ++failures; std::printf("segment %d: FREE\n", b); }
    if (st == LOIKB_MOTION_BLOCKED && !(r.min_sampled[b] < margin + tol && r.s_at_min[b] == r.s_free[b])) { ++failures; std::printf("segment %d: BLOCKED\n", b); }
    if (one.evals[b] != 1 || one.s_free[b] != 0.0 || one.status[b] == LOIKB_MOTION_FREE) { ++failures; std::printf("segment %d: max_evals = 1\n", b); }
  }
  if (!seen[LOIKB_MOTION_FREE] || !seen[LOIKB_MOTION_BLOCKED]) { ++failures; std::printf("outcomes: %d free, %d blocked, %d undecided\n", seen[0], seen[1], seen[2]); }
  // the rows as B / T paths of T samples (the last B % T rows left out)
  const int Bp = B / T;
  const DVec q_path(qa.begin(), qa.begin() + (std::size_t)Bp * T * model.nq);
  const auto p = solver.PathClearance(q_path, T, margin, tol, 16);
  if (p.status.size() != (std::size_t)Bp * (T - 1)) { ++failures; std::printf("PathClearance returned %zu segments\n", p.status.size()); }
  // bad parameters are refused
  int n_threw = 0;
  for (double bad_tol : {0.0, std::nan(""), 1e-10}) {
    try { (void)solver.MotionClearance(qa, dv, margin, bad_tol, 16); } catch (const std::runtime_error&) { ++n_threw; }
  }
  try { (void)solver.MotionClearance(qa, dv, margin, tol, 0); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.PathClearance(q_path, 1, margin, tol, 16); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 5) { ++failures; std::printf("%d of 5 bad calls threw\n", n_threw); }
  DVec all(v);
  append(all, r);
  append(all, one);
  append(all, p);
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all motion checks passed\n");
  return 0;
}

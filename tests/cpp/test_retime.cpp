// Retiming through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_retime.h): Panda-7, the configurations of
// tests/cpp/test_motion.cpp as B / 4 paths of 4 waypoints, limits and a period that are the same doubles in any language.  With a path as
// its argument the program writes what RetimePaths returned there (raw doubles, the integers as doubles), for tests/test_cpp_retime.py
// to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_RETIME_VERSION == 1, "the version of loik_amd_retime.h");
static_assert(sizeof(loikb_retime_params) == 16, "a double, an int and its padding");
static_assert(LOIKB_RETIME_SNAP == 1 && LOIKB_RETIME_TRUNCATED == 1 && LOIKB_RETIME_INVALID == 2 && LOIKB_RETIME_SKIPPED == 4, "the flags");

static void append(DVec& all, const FirstOrderLoikOptimized::RetimeResult& r)
{
  all.push_back(r.S);
  all.insert(all.end(), r.q_traj.begin(), r.q_traj.end());
  all.insert(all.end(), r.v_traj.begin(), r.v_traj.end());
  for (const std::vector<int>* v : {&r.n_samples, &r.n_waypoints, &r.moved, &r.flags}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), r.duration.begin(), r.duration.end());
  all.insert(all.end(), r.seg.begin(), r.seg.end());
}

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_retime_version() != LOIKB_RETIME_VERSION) { ++failures; std::printf("loikb_retime_version() = %d, header %d\n", loikb_retime_version(), LOIKB_RETIME_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67, T = 4, Bp = B / T;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  DVec qa((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  const DVec q_path(qa.begin(), qa.begin() + (std::size_t)Bp * T * model.nq);
  DVec v_max(model.nv), a_max(model.nv);
  for (int j = 0; j < model.nv; ++j) { v_max[j] = 1.0 + j / 8.0; a_max[j] = 2.0 + j / 4.0; }
  const double dt = 1.0 / 32;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);

  const auto r = solver.RetimePaths(q_path, T, v_max, a_max, dt);   // (needs no spheres; S sized by a timing-only call)
  std::vector<int> n_waypoints(Bp);
  for (int b = 0; b < Bp; ++b) n_waypoints[b] = b % (T + 2);   // 0, 1 and T + 1 are skipped
  const auto part = solver.RetimePaths(q_path, T, v_max, a_max, dt, n_waypoints, 64, true);
  const auto timing = solver.RetimePaths(q_path, T, v_max, a_max, dt, {}, 0);
  int longest = 0;
  for (int b = 0; b < Bp; ++b) {
    const int ns = r.n_samples[b];
    longest = std::max(longest, ns);
    if (r.flags[b] != 0 || r.n_waypoints[b] != T || r.moved[b] != T - 1 || ns < 2 || ns > r.S) { ++failures; std::printf("path %d: the info\n", b); continue; }
    if (!(r.duration[b] > (ns - 2) * dt && r.duration[b] <= (ns - 1) * dt)) { ++failures; std::printf("path %d: n_samples against the duration\n", b); }
    if (timing.duration[b] != r.duration[b] || timing.n_samples[b] != ns || timing.flags[b] != 0) { ++failures; std::printf("path %d: the timing-only call\n", b); }
    for (int c = 0; c < model.nq; ++c) {
      const double first = r.q_traj[((std::size_t)b * r.S) * model.nq + c], last = r.q_traj[((std::size_t)b * r.S + ns - 1) * model.nq + c];
      if (first != q_path[((std::size_t)b * T) * model.nq + c] || last != q_path[((std::size_t)b * T + T - 1) * model.nq + c]) { ++failures; std::printf("path %d: the ends\n", b); break; }
    }
    for (int i = 0; i < r.S; ++i)
      for (int j = 0; j < model.nv; ++j)
        if (!(std::fabs(r.v_traj[((std::size_t)b * r.S + i) * model.nv + j]) <= v_max[j] * (1.0 + 1e-12))) { ++failures; std::printf("path %d: v_max at sample %d\n", b, i); i = r.S; break; }
    const int n = n_waypoints[b];
    const bool skip = n < 2 || n > T;
    if (skip != ((part.flags[b] & LOIKB_RETIME_SKIPPED) != 0) || skip != std::isnan(part.duration[b])) { ++failures; std::printf("path %d: n_waypoints = %d\n", b, n); }
    if (!skip && std::fabs(part.duration[b] / dt - std::round(part.duration[b] / dt)) > 1e-9) { ++failures; std::printf("path %d: SNAP\n", b); }
  }
  if (longest != r.S || !timing.q_traj.empty() || part.S != 64) { ++failures; std::printf("the rows: longest %d, S %d\n", longest, r.S); }
  // bad parameters are refused
  int n_threw = 0;
  try { (void)solver.RetimePaths(q_path, T, v_max, a_max, 0.0); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.RetimePaths(q_path, T, DVec(model.nv, 0.0), a_max, dt); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.RetimePaths(q_path, T, v_max, DVec(2, 1.0), dt); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.RetimePaths(q_path, 1, v_max, a_max, dt); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.RetimePaths(q_path, T, v_max, a_max, dt, {1, 2}); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 5) { ++failures; std::printf("%d of 5 bad calls threw\n", n_threw); }
  DVec all;
  append(all, r);
  append(all, part);
  append(all, timing);
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all retime checks passed\n");
  return 0;
}

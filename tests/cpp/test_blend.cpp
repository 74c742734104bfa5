// Certified blends through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_blend.h): Panda-7, the
// configurations, spheres and world of tests/cpp/test_motion.cpp as B / 4 paths of 4 waypoints, limits and a period that are the same
// doubles in any language.  With a path as its argument the program writes what BlendPaths returned there (raw doubles, the integers as
// doubles), for tests/test_cpp_blend.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstddef>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_BLEND_VERSION == 1, "the version of loik_amd_blend.h");
static_assert(sizeof(loikb_blend_params) == 48, "four doubles, three ints and their padding");
static_assert(offsetof(loikb_blend_params, max_evals) == 32 && offsetof(loikb_blend_params, flags) == 40, "the ints follow the doubles");
static_assert(LOIKB_BLEND_TRUNCATED == 1 && LOIKB_BLEND_INVALID == 2 && LOIKB_BLEND_SKIPPED == 4, "the flags");
static_assert(LOIKB_BLEND_TAKEN == 0 && LOIKB_BLEND_BLOCKED == 1 && LOIKB_BLEND_UNDECIDED == 2 && LOIKB_BLEND_COUPLED == 3 &&
              LOIKB_BLEND_ZERO_LEG == 4 && LOIKB_BLEND_OFF == 5, "the statuses");

static void append(DVec& all, const FirstOrderLoikOptimized::BlendResult& r)
{
  all.push_back(r.S);
  all.insert(all.end(), r.q_traj.begin(), r.q_traj.end());
  all.insert(all.end(), r.v_traj.begin(), r.v_traj.end());
  for (const std::vector<int>* v : {&r.n_samples, &r.n_waypoints, &r.taken, &r.flags}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), r.duration.begin(), r.duration.end());
  all.insert(all.end(), r.corner.begin(), r.corner.end());
  all.insert(all.end(), r.corner_info.begin(), r.corner_info.end());
  all.insert(all.end(), r.piece.begin(), r.piece.end());
}

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_blend_version() != LOIKB_BLEND_VERSION) { ++failures; std::printf("loikb_blend_version() = %d, header %d\n", loikb_blend_version(), LOIKB_BLEND_VERSION); }
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
  const double dt = 1.0 / 32, reach = 0.25, margin = -0.0625, tol = 1.0 / 1024;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  bool threw = false;
  try { (void)solver.BlendPaths(q_path, T, v_max, a_max, dt, reach); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("BlendPaths without spheres did not throw\n"); }
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

  const auto r = solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, {}, -1, margin, tol, 16, 3);   // (S sized by a timing-only call)
  std::vector<int> n_waypoints(Bp);
  for (int b = 0; b < Bp; ++b) n_waypoints[b] = b % (T + 2);   // 0, 1 and T + 1 are skipped
  const auto part = solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, n_waypoints, 64, margin, tol, 16, 3);
  const auto timing = solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, {}, 0, margin, tol, 16, 3);
  const auto off = solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, {}, -1, margin, tol, 16, 0);
  const auto stop = solver.RetimePaths(q_path, T, v_max, a_max, dt);
  int longest = 0, taken = 0;
  for (int b = 0; b < Bp; ++b) {
    const int ns = r.n_samples[b];
    longest = std::max(longest, ns);
    if (r.flags[b] != 0 || r.n_waypoints[b] != T || ns < 2 || ns > r.S) { ++failures; std::printf("path %d: the info\n", b); continue; }
    if (!(r.duration[b] > (ns - 2) * dt && r.duration[b] <= (ns - 1) * dt)) { ++failures; std::printf("path %d: n_samples against the duration\n", b); }
    if (timing.duration[b] != r.duration[b] || timing.n_samples[b] != ns || timing.flags[b] != 0) { ++failures; std::printf("path %d: the timing-only call\n", b); }
    int count = 0;
    for (int k = 0; k < T - 2; ++k) {
      const std::size_t c = (std::size_t)b * (T - 2) + k;
      const int st = r.corner_info[6 * c];
      if (st < LOIKB_BLEND_TAKEN || st > LOIKB_BLEND_UNDECIDED) { ++failures; std::printf("path %d corner %d: status %d\n", b, k + 1, st); continue; }
      const bool is_taken = st == LOIKB_BLEND_TAKEN;
      count += is_taken;
      if (is_taken != (r.corner[5 * c] > 0.0) || is_taken != (r.corner[5 * c + 3] > 0.0) || r.corner[5 * c] > reach) { ++failures; std::printf("path %d corner %d: the record\n", b, k + 1); }
      if (is_taken && !(r.corner[5 * c + 4] >= margin + tol)) { ++failures; std::printf("path %d corner %d: min_sampled\n", b, k + 1); }
      if (off.corner_info[6 * c] != LOIKB_BLEND_OFF) { ++failures; std::printf("path %d corner %d: max_tries = 0\n", b, k + 1); }
    }
    taken += count;
    if (count != r.taken[b]) { ++failures; std::printf("path %d: the count of corners taken\n", b); }
    if (count > 0 && !(r.duration[b] <= stop.duration[b])) { ++failures; std::printf("path %d: slower than RetimePaths\n", b); }
    if (!(std::fabs(off.duration[b] - stop.duration[b]) <= 1e-12 * (1.0 + stop.duration[b])) || off.n_samples[b] != stop.n_samples[b]) { ++failures; std::printf("path %d: max_tries = 0 against RetimePaths\n", b); }
    for (int c = 0; c < model.nq; ++c) {
      const double first = r.q_traj[((std::size_t)b * r.S) * model.nq + c], last = r.q_traj[((std::size_t)b * r.S + ns - 1) * model.nq + c];
      if (first != q_path[((std::size_t)b * T) * model.nq + c] || last != q_path[((std::size_t)b * T + T - 1) * model.nq + c]) { ++failures; std::printf("path %d: the ends\n", b); break; }
    }
    for (int i = 0; i < r.S; ++i)
      for (int j = 0; j < model.nv; ++j)
        if (!(std::fabs(r.v_traj[((std::size_t)b * r.S + i) * model.nv + j]) <= v_max[j] * (1.0 + 1e-12))) { ++failures; std::printf("path %d: v_max at sample %d\n", b, i); i = r.S; break; }
    const int n = n_waypoints[b];
    const bool skip = n < 2 || n > T;
    if (skip != ((part.flags[b] & LOIKB_BLEND_SKIPPED) != 0) || skip != std::isnan(part.duration[b])) { ++failures; std::printf("path %d: n_waypoints = %d\n", b, n); }
  }
  if (longest != r.S || !timing.q_traj.empty() || part.S != 64) { ++failures; std::printf("the rows: longest %d, S %d\n", longest, r.S); }
  if (taken == 0) { ++failures; std::printf("no corner was taken\n"); }
  // bad parameters are refused
  int n_threw = 0;
  try { (void)solver.BlendPaths(q_path, T, v_max, a_max, 0.0, reach); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, T, v_max, a_max, dt, 0.0); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, T, DVec(model.nv, 0.0), a_max, dt, reach); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, T, v_max, DVec(2, 1.0), dt, reach); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, 1, v_max, a_max, dt, reach); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, {1, 2}); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.BlendPaths(q_path, T, v_max, a_max, dt, reach, {}, -1, margin, tol, 16, 17); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 7) { ++failures; std::printf("%d of 7 bad calls threw\n", n_threw); }
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
  std::printf("all blend checks passed\n");
  return 0;
}

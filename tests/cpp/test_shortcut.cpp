// Shortcutting through the C++ mirror (include/loik_amd/loik.hpp, which includes include/loik_amd_shortcut.h): Panda-7, two spheres per
// link, a world of two spheres and one box, self pairs; the configurations of tests/cpp/test_motion.cpp as B / 4 paths of 4 waypoints.
// With a path as its argument the program writes what ShortcutPaths and PathLength returned there (raw doubles, the integers as
// doubles), for tests/test_cpp_shortcut.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;

static_assert(LOIKB_SHORTCUT_VERSION == 1, "the version of loik_amd_shortcut.h");
static_assert(sizeof(loikb_shortcut_params) == 40, "two doubles, two ints, a 64-bit seed, an int and its padding");

static void append(DVec& all, const FirstOrderLoikOptimized::ShortcutResult& r)
{
  all.insert(all.end(), r.q_path.begin(), r.q_path.end());
  for (const std::vector<int>* v : {&r.n_waypoints, &r.keep, &r.tried, &r.accepted, &r.blocked, &r.undecided, &r.invalid}) all.insert(all.end(), v->begin(), v->end());
  all.insert(all.end(), r.length_in.begin(), r.length_in.end());
  all.insert(all.end(), r.length_out.begin(), r.length_out.end());
}

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_shortcut_version() != LOIKB_SHORTCUT_VERSION) { ++failures; std::printf("loikb_shortcut_version() = %d, header %d\n", loikb_shortcut_version(), LOIKB_SHORTCUT_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67, T = 4, Bp = B / T;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations that are the same doubles in any language: sixteenths
  DVec qa((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) qa[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  const DVec q_path(qa.begin(), qa.begin() + (std::size_t)Bp * T * model.nq);
  bool threw = false;
  try { (void)solver.ShortcutPaths(q_path, T); } catch (const std::runtime_error&) { threw = true; }
  if (!threw) { ++failures; std::printf("ShortcutPaths without spheres did not throw\n"); }
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(qa, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const DVec length = solver.PathLength(q_path, T);   // (needs no spheres)
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
  const double margin = -0.0625, tol = 1.0 / 1024;
  const auto r = solver.ShortcutPaths(q_path, T, {}, 6, 99ull, margin, tol, 64);
  std::vector<int> n_waypoints(Bp);
  for (int b = 0; b < Bp; ++b) n_waypoints[b] = b % (T + 2);   // 0, 1 and T + 1 are skipped
  const auto part = solver.ShortcutPaths(q_path, T, n_waypoints, 6, 99ull, margin, tol, 64);
  const DVec part_length = solver.PathLength(q_path, T, n_waypoints);
  int accepted = 0, refused = 0;
  for (int b = 0; b < Bp; ++b) {
    const int L = r.n_waypoints[b];
    accepted += r.accepted[b];
    refused += r.blocked[b] + r.undecided[b];
    if (L < 2 || L > T || r.keep[(std::size_t)b * T] != 0 || r.keep[(std::size_t)b * T + L - 1] != T - 1) { ++failures; std::printf("path %d: L / the ends\n", b); continue; }
    if (r.tried[b] != r.accepted[b] + r.blocked[b] + r.undecided[b] + r.invalid[b] || r.invalid[b] != 0) { ++failures; std::printf("path %d: the counters\n", b); }
    if (r.length_in[b] != length[b] || !(r.length_out[b] <= r.length_in[b])) { ++failures; std::printf("path %d: the lengths\n", b); }
    for (int k = 0; k < T; ++k) {
      const int src = r.keep[(std::size_t)b * T + (k < L ? k : L - 1)];
      if (k >= L && r.keep[(std::size_t)b * T + k] != -1) { ++failures; std::printf("path %d: keep after L\n", b); }
      for (int c = 0; c < model.nq; ++c)
        if (r.q_path[((std::size_t)b * T + k) * model.nq + c] != q_path[((std::size_t)b * T + src) * model.nq + c]) { ++failures; std::printf("path %d: row %d\n", b, k); break; }
    }
    const int n = n_waypoints[b];
    if ((n < 2 || n > T) != (part.n_waypoints[b] == 0) || (n > T) != std::isnan(part_length[b])) { ++failures; std::printf("path %d: n_waypoints = %d\n", b, n); }
  }
  if (!accepted || !refused) { ++failures; std::printf("outcomes: %d accepted, %d refused\n", accepted, refused); }
  // bad parameters are refused
  int n_threw = 0;
  try { (void)solver.ShortcutPaths(q_path, T, {}, -1); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.ShortcutPaths(q_path, T, {}, 6, 0ull, margin, 0.0); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.ShortcutPaths(q_path, 1); } catch (const std::runtime_error&) { ++n_threw; }
  try { (void)solver.PathLength(q_path, T, {1, 2}); } catch (const std::runtime_error&) { ++n_threw; }
  if (n_threw != 4) { ++failures; std::printf("%d of 4 bad calls threw\n", n_threw); }
  DVec all(length);
  append(all, r);
  append(all, part);
  all.insert(all.end(), part_length.begin(), part_length.end());
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all shortcut checks passed\n");
  return 0;
}

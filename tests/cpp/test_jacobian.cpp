// Frame Jacobians, dexterity and the dexterous multi-start latch through the C++ mirror (include/loik_amd/loik.hpp, which includes
// include/loik_amd_jacobian.h): Panda-7, two links with tool frames.  With a path as its argument the program writes what the three
// calls returned there (raw doubles: FrameJacobians in the three reference frames, FrameDexterity, TaskDexterity), for
// tests/test_cpp_jacobian.py to compare with the Python binding bit for bit.  Exit code 0 = all checks passed.  Needs a GPU.
#include "loik_amd/loik.hpp"

#include <cmath>
#include <cstdio>

using namespace loik_amd;
using SE3 = FirstOrderLoikOptimized::SE3;

static_assert(LOIKB_JAC_LOCAL == 0 && LOIKB_JAC_LOCAL_WORLD_ALIGNED == 1 && LOIKB_JAC_WORLD == 2, "the reference frames of loik_amd_jacobian.h");
static_assert(LOIKB_DEX_SIGMA5 == 5 && LOIKB_DEX_MANIPULABILITY == 6 && LOIKB_DEX_INV_CONDITION == 7 && LOIKB_DEX_N == 8, "the dexterity record");

int main(int argc, char** argv)
{
  int failures = 0;
  if (loikb_jacobian_version() != LOIKB_JACOBIAN_VERSION) { ++failures; std::printf("loikb_jacobian_version() = %d, header %d\n", loikb_jacobian_version(), LOIKB_JACOBIAN_VERSION); }
  const Model model = Model::Builtin("panda7");
  const int B = 67;
  const Index ee = 7;
  IkIdDataOptimized data(model, 1, B);
  FirstOrderLoikOptimized solver(300, 1e-6, 0.0, 1e-2, 1e-2, 1e-5, 1e-2, 1e4, DEFAULT, 1, 6, model, data, true, 1e-1, false, false);
  // configurations that are the same doubles in any language: sixteenths
  DVec q_t(model.nq, 0.25), q0((std::size_t)B * model.nq);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < model.nq; ++k) q0[(std::size_t)b * model.nq + k] = ((b * 7 + 3 * k) % 17 - 8) / 16.0;
  std::vector<Mat6x6> A{Identity6()};
  std::vector<Vec6> bis{Vec6{}};
  DVec lb(model.nv, -2.0), ub(model.nv, 2.0);
  solver.SolveInit(q_t, Identity6(), Motion{}, {ee}, A, bis, lb, ub);
  const SE3 tool{0, -1, 0, 1, 0, 0, 0, 0, 1, 0.125, 0.0, 0.25}, elbow{1, 0, 0, 0, 0, -1, 0, 1, 0, 0.0, 0.5, 0.0};
  const SE3 D = solver.FramePlacements({ee}, {tool})[0];
  (void)solver.SolvePose({D}, 1.0, 1.0, 1e-6, 0, &q0);   // no step: the resident q is q0
  const std::vector<Index> links{ee, 4};
  const std::vector<SE3> frames{tool, elbow};
  DVec all;
  const std::size_t nJ = (std::size_t)B * 2 * 6 * model.nv;
  for (int ref : {LOIKB_JAC_LOCAL, LOIKB_JAC_LOCAL_WORLD_ALIGNED, LOIKB_JAC_WORLD}) {
    const DVec J = solver.FrameJacobians(links, frames, ref);
    if (J.size() != nJ) { ++failures; std::printf("FrameJacobians returned %zu doubles, expected %zu\n", J.size(), nJ); }
    // the last link's own DoF turns about the joint's z axis: seen from the tool frame (a quarter turn about z) still its z axis
    if (ref == LOIKB_JAC_LOCAL && !(J[(5 * (std::size_t)model.nv) + 6] == 1.0 && J[(3 * (std::size_t)model.nv) + 6] == 0.0)) { ++failures; std::printf("the wrist column is not the tool's z axis\n"); }
    // link 4 does not move with joints 5..7
    for (int r = 0; r < 6; ++r)
      for (int k = 4; k < 7; ++k)
        if (J[((std::size_t)(1 * 6 + r)) * model.nv + k] != 0.0) { ++failures; std::printf("an off-path column is not zero\n"); }
    all.insert(all.end(), J.begin(), J.end());
  }
  const DVec dex = solver.FrameDexterity(links, frames, {0x3f, 0x07}, 0.5);
  if (dex.size() != (std::size_t)B * 2 * LOIKB_DEX_N) { ++failures; std::printf("FrameDexterity returned %zu doubles\n", dex.size()); }
  for (int b = 0; b < B; ++b) {
    const double* d = &dex[((std::size_t)b * 2 + 1) * LOIKB_DEX_N];
    if (!(d[0] >= d[1] && d[1] >= d[2] && d[2] > 0.0 && d[3] == 0.0 && d[4] == 0.0 && d[5] == 0.0)) { ++failures; std::printf("instance %d: the position task has no three singular values\n", b); }
    if (std::fabs(d[LOIKB_DEX_INV_CONDITION] - d[2] / d[0]) > 1e-14) { ++failures; std::printf("instance %d: inv_condition\n", b); }
  }
  all.insert(all.end(), dex.begin(), dex.end());
  solver.setPoseTasks({LOIKB_TASK_POSITION}, {tool});
  const DVec tdex = solver.TaskDexterity(0.5);
  const DVec want = solver.FrameDexterity({ee}, {tool}, {0x07}, 0.5);
  if (tdex != want) { ++failures; std::printf("TaskDexterity differs from the explicit call\n"); }
  all.insert(all.end(), tdex.begin(), tdex.end());
  // the latch
  if (solver.MultiStartPickDexterous() != 0.0) { ++failures; std::printf("a latch before any was set\n"); }
  solver.setMultiStartPickDexterous(0.75);
  if (solver.MultiStartPickDexterous() != 0.75) { ++failures; std::printf("the latch does not return what was set\n"); }
  int n_threw = 0;
  for (double bad : {0.0, -1.0, std::nan("")}) {
    try { solver.setMultiStartPickDexterous(bad); } catch (const std::runtime_error&) { ++n_threw; }
  }
  if (n_threw != 3 || solver.MultiStartPickDexterous() != 0.75) { ++failures; std::printf("%d of 3 bad lengths threw, latch %g\n", n_threw, solver.MultiStartPickDexterous()); }
  solver.clearMultiStartPickDexterous();
  if (solver.MultiStartPickDexterous() != 0.0) { ++failures; std::printf("the latch was not cleared\n"); }
  // no links: empty results, nothing thrown
  if (!solver.FrameJacobians({}).empty() || !solver.FrameDexterity({}).empty()) { ++failures; std::printf("no links gave a result\n"); }
  try { (void)solver.FrameJacobians({ee}, {}, 3); ++failures; std::printf("reference frame 3 was accepted\n"); } catch (const std::runtime_error&) {}
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(all.data(), sizeof(double), all.size(), f) != all.size()) { ++failures; std::printf("cannot write %s\n", argv[1]); }
    if (f) std::fclose(f);
  }
  if (failures) return 1;
  std::printf("all jacobian checks passed\n");
  return 0;
}

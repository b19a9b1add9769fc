// Runs the pyramid build planner (csrc/build_plan.h) on a CPU for
// tests/test_build_plan.py.  Reads one request per line from the file named by
// argv[1]:
//   in_dtype layout B D H W num_levels divisor pyr_dtype algo fmap1 fmap2 pyramid workspace
//   workspace_bytes
// (addresses as unsigned integers; divisor as a float, "nan" accepted) and prints
//   status <tab> path name <tab> dxr_build_workspace_bytes <tab> operand cells pool_extra
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "build_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char div[64];
  dxr::BuildRequest r;
  uint64_t p[4];
  while (std::fscanf(f, "%d %d %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %63s %d %d %" SCNu64
                        " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64,
                     &r.in_dtype, &r.fmap_layout, &r.B, &r.D, &r.H, &r.W, &r.num_levels, div,
                     &r.pyr_dtype, &r.algo, &p[0], &p[1], &p[2], &p[3], &r.workspace_bytes) == 15) {
    r.divisor = std::strtof(div, nullptr);
    r.fmap1 = (uintptr_t)p[0];
    r.fmap2 = (uintptr_t)p[1];
    r.pyramid = (uintptr_t)p[2];
    r.workspace = (uintptr_t)p[3];
    dxr::BuildPlan plan;
    const int st = dxr::plan_build(r, &plan);
    std::printf("%d\t%s\t%" PRId64 "\t%d %d %d\n", st, dxr::build_path_name(plan.path),
                dxr::build_workspace_bytes(r.in_dtype, r.B, r.D, r.H, r.W), plan.operand, plan.cells,
                (int)plan.pool_extra);
  }
  const bool whole = std::feof(f) != 0;
  std::fclose(f);
  return whole ? 0 : 3;   // 3: a line did not parse
}

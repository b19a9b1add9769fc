// Runs the lookup planner (csrc/lookup_plan.h) on a CPU for
// tests/test_lookup_plan.py.  Reads one request per line from the file named by
// argv[1], the first word naming the family:
//   P pyr_dtype B H W num_levels radius conv1x1 cout pyramid coords weight_packed out
//   V B H W num_levels first_level radius divisor volumes coords out
//   A B H W C num_levels n_levels levels_call radius divisor fmap1 fmap2_levels coords out
//     workspace workspace_bytes level0 ... level7
// (addresses as unsigned integers; divisor as a float, "nan" accepted) and prints
//   status <tab> unit <tab> kernel name <tab> cells out_flag nhwc radius gx gy gz out_nt
// for P and V (cells: the dxr_dtype of the cells read), and for A
//   status <tab> unit <tab> kernel name <tab> out_flag nhwc radius levels use_workspace
//     dxr_alt_workspace_bytes(B, H, W, num_levels)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "lookup_plan.h"

static bool addresses(std::FILE* f, int n, uintptr_t* out) {
  for (int i = 0; i < n; ++i) {
    uint64_t v;
    if (std::fscanf(f, "%" SCNu64, &v) != 1) return false;
    out[i] = (uintptr_t)v;
  }
  return true;
}

static void print_launch(int st, const char* unit, const char* name, int cells, int out_flag, bool nhwc,
                         int radius, const dxr::LookupLaunch& s) {
  std::printf("%d\t%s\t%s\t%d %d %d %d %u %u %u %d\n", st, unit, name, cells, out_flag, (int)nhwc,
              radius, s.gx, s.gy, s.gz, s.out_nt);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char fam[8], div[64];
  bool ok = true;
  while (ok && std::fscanf(f, "%7s", fam) == 1) {
    uintptr_t p[14];
    if (fam[0] == 'P') {
      dxr::LookupRequest r;
      int conv;
      ok = std::fscanf(f, "%d %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %d %d %" SCNd64, &r.pyr_dtype, &r.B,
                       &r.H, &r.W, &r.num_levels, &r.radius, &conv, &r.cout) == 8 &&
           addresses(f, 4, p);
      if (!ok) break;
      r.conv1x1 = conv != 0;
      r.pyramid = p[0];
      r.coords = p[1];
      r.weight_packed = p[2];
      r.out = p[3];
      dxr::LookupPlan plan;
      const int st = dxr::plan_lookup(r, &plan);
      print_launch(st, dxr::lookup_unit_name(plan.unit), dxr::lookup_name(plan), plan.cells,
                   plan.out_flag, plan.nhwc, plan.radius, plan.launch);
    } else if (fam[0] == 'V') {
      dxr::VolumeLookupRequest r;
      ok = std::fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %d %d %d %63s", &r.B, &r.H, &r.W,
                       &r.num_levels, &r.first_level, &r.radius, div) == 7 &&
           addresses(f, 3, p);
      if (!ok) break;
      r.divisor = std::strtof(div, nullptr);
      r.volumes = p[0];
      r.coords = p[1];
      r.out = p[2];
      dxr::VolumeLookupPlan plan;
      const int st = dxr::plan_volume_lookup(r, &plan);
      print_launch(st, dxr::volume_unit_name(plan.unit), dxr::volume_lookup_name(plan), plan.cells,
                   plan.out_flag, plan.nhwc, plan.radius, plan.launch);
    } else if (fam[0] == 'A') {
      dxr::AltLookupRequest r;
      int levels_call;
      ok = std::fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %d %d %d %d %63s", &r.B, &r.H,
                       &r.W, &r.C, &r.num_levels, &r.n_levels, &levels_call, &r.radius, div) == 9 &&
           addresses(f, 5, p) && std::fscanf(f, "%" SCNd64, &r.workspace_bytes) == 1 &&
           addresses(f, 8, r.level);
      if (!ok) break;
      r.levels_call = levels_call != 0;
      r.divisor = std::strtof(div, nullptr);
      r.fmap1 = p[0];
      r.fmap2_levels = p[1];
      r.coords = p[2];
      r.out = p[3];
      r.workspace = p[4];
      dxr::AltLookupPlan plan;
      const int st = dxr::plan_alt_lookup(r, &plan);
      std::printf("%d\t%s\t%s\t%d %d %d %d %d %" PRId64 "\n", st, dxr::alt_unit_name(plan.unit),
                  dxr::alt_lookup_name(plan), plan.out_flag, (int)plan.nhwc, plan.radius, plan.levels,
                  (int)plan.use_workspace, dxr::alt_workspace_bytes(r.B, r.H, r.W, r.num_levels));
    } else {
      ok = false;
    }
  }
  const bool whole = ok && std::feof(f) != 0;
  std::fclose(f);
  return whole ? 0 : 3;   // 3: a line did not parse
}

// extern "C" face of rsparse_amd/csrc/wrmf_schedule.cpp for tests/test_cgp_quad_schedule.py (compiled with g++ into pytest's
// tmp_path, like tests/schedule_wide_shim.cpp): grid, visits per wave and loss slots of a short-row launch of wrmf_cgp.hip.
#include <cstdint>

#include "../rsparse_amd/csrc/wrmf_schedule.h"

using namespace rsparse_hip;

extern "C" {

// out = {workgroups, visits per wave, loss slots} of a launch over n_rows rows, rows_per_wave rows of the list per wave visit
void cgp_launch_plan(int n_rows, int rows_per_wave, int64_t out[3]) {
  out[0] = cgp_grid(n_rows, rows_per_wave);
  out[1] = cgp_visits(n_rows, rows_per_wave);
  out[2] = cgp_loss_slots(n_rows, rows_per_wave);
}

}  // extern "C"

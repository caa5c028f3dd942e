// lcv_k_rlc.hip — kernel unit: F_rlc_scale F_rlc_spread F_sop_lines_g1 F_sop_f12mul F_sop_fexp_rows and the test
// hooks' functors, randomised batch verification (lcv_rlc.hpp; see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_rlc.hpp"

LCV_INSTANTIATE(F_rlc_scale)
LCV_INSTANTIATE(F_rlc_spread)
LCV_INSTANTIATE(F_dbg_rlc_coeffs)
LCV_INSTANTIATE(F_dbg_rlc_scale)
LCV_INSTANTIATE_SOP(F_sop_lines_g1)
LCV_INSTANTIATE_SOP(F_sop_f12mul)
LCV_INSTANTIATE_SOP_COUNTED(F_sop_fexp_rows)

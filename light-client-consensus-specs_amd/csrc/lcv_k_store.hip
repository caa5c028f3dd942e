// lcv_k_store.hip — kernel unit: F_nsc_eq_team F_pre_table, the store-table path of validate (see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_functors.hpp"

LCV_INSTANTIATE_TEAM(F_nsc_eq_team)
LCV_INSTANTIATE(F_pre_table)

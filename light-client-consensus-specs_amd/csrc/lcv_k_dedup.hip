// lcv_k_dedup.hip — kernel unit: F_dedup_gather F_verdict_dedup, the deduplicated BLS half of validate, and F_dedup_key
// F_dedup_confirm, the classes of a resident batch (lcv_dedup.hpp; see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_dedup.hpp"

LCV_INSTANTIATE_TEAM(F_dedup_gather)
LCV_INSTANTIATE(F_verdict_dedup)
LCV_INSTANTIATE_TEAM(F_dedup_key)
LCV_INSTANTIATE_TEAM(F_dedup_confirm)

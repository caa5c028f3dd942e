// lcv_k_fold.hip — kernel unit: F_rank F_fold F_fold_seg, the store fold behind validate (lcv_fold.hpp; see
// lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_functors.hpp"

LCV_INSTANTIATE(F_rank)
LCV_INSTANTIATE_TEAM(F_fold)
LCV_INSTANTIATE_TEAM(F_fold_seg)

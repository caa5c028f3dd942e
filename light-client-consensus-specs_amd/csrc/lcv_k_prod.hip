// lcv_k_prod.hip — kernel unit: F_prod_block F_prod_state F_prod_rows F_prod_pick F_prod_boot (the producer side,
// lcv_producer.hpp; see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_producer.hpp"

LCV_INSTANTIATE(F_prod_block)
LCV_INSTANTIATE(F_prod_state)
LCV_INSTANTIATE_TEAM(F_prod_rows)
LCV_INSTANTIATE_TEAM(F_prod_pick)
LCV_INSTANTIATE_TEAM(F_prod_boot)

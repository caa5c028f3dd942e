// lcv_k_dec.hip — kernel unit: F_wire_dec, F_sc_confirm, F_sc_gather (SSZ wire messages into a resident batch,
// lcv_wire_dec.hpp; see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_wire_dec.hpp"

LCV_INSTANTIATE_TEAM(F_wire_dec)
LCV_INSTANTIATE_TEAM(F_sc_confirm)
LCV_INSTANTIATE_TEAM(F_sc_gather)

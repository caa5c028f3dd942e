// lcv_k_enc.hip — kernel unit: F_wire_enc (SSZ wire bytes of a resident batch, lcv_wire_enc.hpp; see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_wire_enc.hpp"

LCV_INSTANTIATE_TEAM(F_wire_enc)

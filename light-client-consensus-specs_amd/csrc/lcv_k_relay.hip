// lcv_k_relay.hip — kernel unit: F_wire_relay (the asynchronous relay's decode through a row map, lcv_wire_dec.hpp;
// see lcv_launch.hpp).
#define LCV_KERNEL_UNIT 1
#define LCV_HD __device__
#include "lcv_launch.hpp"
#include "lcv_wire_dec.hpp"

LCV_INSTANTIATE_TEAM(F_wire_relay)

// What the device code (common.hpp) and the host-only headers (eqds_host.hpp, cg_host.hpp) share without a HIP header: the status codes of the
// C ABI (CMBL_ERR_* of include/cmblens.h) and the largest batch.
#pragma once
namespace cmbl {
enum Status { OK = 0, ERR_ARG = 1, ERR_SHAPE = 2, ERR_HIP = 3, ERR_NAN = 4, ERR_STATE = 5, ERR_ALLOC = 6 };
constexpr int MAXBATCH = 256;                  // most batch slots (chains per GPU) a reduction / CG / posterior call takes: sizes the per-slot scalar buffers
}  // namespace cmbl

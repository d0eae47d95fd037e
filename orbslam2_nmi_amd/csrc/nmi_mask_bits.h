// nmi_mask_bits.h -- internal interface of the bit-packed mask kernels (nmi_mask_bits.hip), used by nmi_capi_pipeline.cpp
// (covered stream tickets: render masks cross PCIe as bits) and nmi_capi_covered.cpp (nmi_pack_mask_bits).
//
// Layout (include/nmi_hip.h, nmi_pack_mask_bits): image i of n occupies mask_bit_bytes(npix) bytes; pixel p (row-major, in the
// image's own layout) is bit p % 8 (LSB first) of byte p / 8; bits past npix in the last byte are 0 when packed, ignored when read.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nmi {

inline size_t mask_bit_bytes(int npix) { return ((size_t)npix + 7) / 8; }

// out[i][p] = bit p of image i's bits, as a byte 0 / 1.  16-byte stores (one per lane per 16 pixels) where npix % 16 == 0 and
// out is 16-byte aligned; a byte per lane otherwise.
hipError_t launch_unpack_mask_bits(const uint8_t *bits, int n, int npix, uint8_t *out, hipStream_t stream);
// bits[i][j] = (masks[i][8j + k] != 0) << k for the pixels 8j + k < npix (0 above); one bit byte per lane.
hipError_t launch_pack_mask_bits(const uint8_t *masks, int n, int npix, uint8_t *bits, hipStream_t stream);

}  // namespace nmi

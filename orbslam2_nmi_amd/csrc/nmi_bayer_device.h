// nmi_bayer_device.h -- device code of the Bayer-mosaic-to-grey rule (nmi_gray_frame, include/nmi_hip.h) of the mosaic kernel
// (nmi_bayer.hip: conversion and reduction).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nmi {
namespace {

// The grey value of one mosaic site: a bilinear demosaic (R4, G4, B4 are four times the channels) and nmi_gray_frame's weights
// with one rounding.  c = p(0,0), hs = p(-1,0) + p(1,0), vs = p(0,-1) + p(0,1), ds = the four diagonal neighbours' sum; a, b =
// 0 where the site's column / row has the parity of the red sites' (a = b = 0: red, a = b = 1: blue, a != b: green, in a red
// row when b = 0).  The weights sum to 2^14, so a flat mosaic of value g gives g exactly.
__device__ __forceinline__ uint32_t bayer_gray(uint32_t c, uint32_t hs, uint32_t vs, uint32_t ds, int a, int b)
{
    const bool green = a != b;
    const uint32_t g4 = green ? 4u * c : hs + vs;
    const uint32_t same = green ? 2u * hs : 4u * c;  // the colour of this row's non-green sites
    const uint32_t other = green ? 2u * vs : ds;     // the colour of the rows above and below
    const uint32_t r4 = b == 0 ? same : other, b4 = b == 0 ? other : same;
    return (4899u * r4 + 9617u * g4 + 1868u * b4 + 32768u) >> 16;
}

// Coordinate i of 0 .. n-1, reflected without repeating the edge (-1 -> 1, n -> n - 2; n >= 2), so that the mosaic keeps its
// colour phase.
__device__ __forceinline__ int bayer_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

}  // namespace
}  // namespace nmi

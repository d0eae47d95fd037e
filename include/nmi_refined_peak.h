/*
 * nmi_refined_peak.h -- the record of a refined peak and its flags, shared by nmi_hip.h (nmi_refine_peaks, the device form) and
 * nmi_host.h (nmi_refine_peaks_host, the host twin).  The rule that fills it is nmi_hip.h's section "Refined peaks".
 */
#ifndef NMI_REFINED_PEAK_H
#define NMI_REFINED_PEAK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nmi_refined_peak {
    uint64_t key;        /* the key as given; 0: no peak (the whole record is 0 but for flags = NMI_REFINE_EMPTY) */
    float    offset[6];  /* cells, in [-1, 1]; 0 on an inactive axis */
    float    score;      /* the quadratic's value at the offset (NaN if sums of samples overflowed fp32; the offsets stay in range) */
    uint32_t flags;      /* NMI_REFINE_* */
    float    gradient[6];
    float    hessian[21];/* upper triangle, row-major (0,0) (0,1) .. (0,5) (1,1) ..; 0 for inactive axes */
    uint32_t reserved;   /* 0 */
} nmi_refined_peak;      /* 152 bytes */

#define NMI_REFINE_EMPTY      0x00000001u /* key 0, or an index that is not a cell of the table: nothing was read */
#define NMI_REFINE_NONFINITE  0x00000002u /* the centre is not usable (+inf): offsets 0, score = the centre */
#define NMI_REFINE_COUPLED    0x00000004u /* the offset is the coupled step; else each axis went on its own */
#define NMI_REFINE_CROSS_HOLE 0x00000008u /* a cross term of two active axes was set to 0: a corner was not usable */
#define NMI_REFINE_BORDER(a)  (0x00000100u << (a)) /* the peak is on the first or last cell of axis a (num[a] >= 2) */
#define NMI_REFINE_HOLE(a)    (0x00010000u << (a)) /* an axial neighbour on axis a is not usable */
#define NMI_REFINE_FLAT(a)    (0x01000000u << (a)) /* separable step: H_aa >= 0, offset 0 */

#ifdef __cplusplus
}
#endif
#endif /* NMI_REFINED_PEAK_H */

// nmi_clahe_valid.hip -- nmi_clahe.hip's histogram and conversion kernels once more, as nmi_clahe_hist_ranged_kernel and
// nmi_clahe_gray16_masked_kernel with their launches (nmi_tone.h): the forms a valid range takes (nmi_set_valid_range).  See the
// comment at the head of nmi_clahe.hip.
#define NMI_CLAHE_VALID 1
#include "nmi_clahe.hip"

// nmi_tone_valid.hip -- nmi_tone.hip's histogram and conversion kernels once more, as nmi_tone_hist_ranged_kernel and
// nmi_gray16_masked_kernel with their launches (nmi_tone.h): the forms a valid range takes (nmi_set_valid_range).  See the comment at
// the head of nmi_tone.hip.
#define NMI_TONE_VALID 1
#include "nmi_tone.hip"

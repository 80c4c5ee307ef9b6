// the unit of the operand-free mode-2 instance k_conv_fft<3, false> (see the SEL part of ics_conv_fft.hip and ics_maxg_select.h)
#define ICS_FFT_SEL_UNIT 1
#include "ics_conv_fft.hip"

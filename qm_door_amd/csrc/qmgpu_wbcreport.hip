// wbc_report_kernel in a translation unit of its own (qm_door_amd/build.py; qmgpu_api.hip only declares the kernel, QM_WBCREPORT_EXTERN, and launches it), for the
// reason qmgpu_plant.hip gives: the translation units of the other kernels compile from the input they had before this kernel existed, and wbc_kernel's results
// have depended on what it was compiled next to.  This kernel calls wbc_kernel.h's device functions, so it includes that header; the copy
// of wbc_kernel the header defines is compiled here once more and never launched, under a kernel namespace renamed by build.py (-Dqmk=qmkreport).
// linesearch_kernel.h, which wbc_kernel.h includes for DblIn, only declares its kernel here.
#define QM_LS_EXTERN
#include "kernels/wbc_report_kernel.h"

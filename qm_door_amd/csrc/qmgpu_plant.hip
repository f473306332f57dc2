// plant_kernel in a translation unit of its own (qm_door_amd/build.py; qmgpu_api.hip only declares the kernel, QM_PLANT_EXTERN, and launches it): the translation
// units of the other kernels compile from the input they had before this kernel existed.  wbc_kernel's results have depended on what it was compiled next to twice
// (DESIGN.md section 4.7.1), and this kernel calls wbc_kernel.h's device functions, so it includes that header.  What the header defines besides them -- wbc_kernel
// itself -- is compiled here a second time and never launched; build.py renames the kernel namespace of this unit (-Dqmk=qmkplant, as qmgpu_mpc32.hip's qmk32) so that the
// copy does not collide with the product's.  linesearch_kernel.h, which wbc_kernel.h includes for DblIn, only declares its kernel here.
#define QM_LS_EXTERN
#include "kernels/plant_kernel.h"

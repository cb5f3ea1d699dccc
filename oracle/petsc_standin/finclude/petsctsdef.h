! petsctsdef.h -- stand-in: the hot-path sources include this name at module
! scope for the macros of petscdef.h, which the PETSc header of this name
! brings with it; nothing else of it is used.
#include "finclude/petscdef.h"

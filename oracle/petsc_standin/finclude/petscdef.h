! petscdef.h -- one-rank stand-in for the PETSc header of this name.
! Macros only, so that it can be included at module scope: the handle and
! number types the hot-path sources declare their variables with.
! TEST INFRASTRUCTURE ONLY (oracle/Makefile, target ref).
#ifndef PIC1DP_STANDIN_PETSCDEF_H
#define PIC1DP_STANDIN_PETSCDEF_H
#define Vec integer(kind=8)
#define Mat integer(kind=8)
#define IS integer(kind=8)
#define VecScatter integer(kind=8)
#define PetscViewer integer(kind=8)
#define PetscInt integer(kind=4)
#define PetscErrorCode integer(kind=4)
#define PetscBool logical(kind=4)
#define PetscReal real(kind=8)
#define PetscScalar real(kind=8)
#define MATAIJ 'aij'
#define CHKERRQ(n) if (n .ne. 0) stop 86
#endif

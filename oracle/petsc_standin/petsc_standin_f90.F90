! petsc_standin_f90.F90 -- the two stand-in entry points that hand a Fortran
! pointer to a vector's storage (interfaces: finclude/petsc.h90); the rest of
! the stand-in is petsc_standin.c.  TEST INFRASTRUCTURE ONLY.
subroutine VecGetArrayF90(v, a, ierr)
  use iso_c_binding
  implicit none
  integer(kind=8), intent(in) :: v
  real(kind=8), dimension(:), pointer :: a
  integer(kind=4), intent(out) :: ierr
  type(c_ptr) :: raw
  integer(kind=8) :: n
  external :: standin_vec_raw
  call standin_vec_raw(v, raw, n)
  call c_f_pointer(raw, a, (/ n /))
  ierr = 0
end subroutine VecGetArrayF90

subroutine VecRestoreArrayF90(v, a, ierr)
  implicit none
  integer(kind=8), intent(in) :: v
  real(kind=8), dimension(:), pointer :: a
  integer(kind=4), intent(out) :: ierr
  nullify (a)
  ierr = 0
end subroutine VecRestoreArrayF90

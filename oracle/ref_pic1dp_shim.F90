! ref_pic1dp_shim.F90 -- bind(C) entry points around the REFERENCE's own
! hot-path modules (pic1dp_global, wtimer, pic1dp_field, pic1dp_particle,
! pic1dp_interaction), compiled where they lie against the serial stand-in in
! oracle/petsc_standin and an input module written by oracle/gen_ref_input.py
! (see oracle/Makefile).  One library per configuration: the reference's inputs
! are compile-time parameters.  Test infrastructure only: it lets tests/ and the
! fixture generator run the reference's own statements to pin the restatement
! in pic1dp_oracle.c and the kernels.  This file contains no reference source
! text.
module ref_pic1dp_shim
use iso_c_binding
use multirand
use pic1dp_global
use pic1dp_input
use pic1dp_field
use pic1dp_particle
use pic1dp_interaction
implicit none
contains

! one rank; the objects of particle_init and field_init; time zero
subroutine ref_init() bind(C, name="ref_init")
  global_mype = 0
  global_npe = 1
  global_ierr = 0
  global_itime = 0
  global_time = 0.0_kpr
  global_irk = 1
  call particle_init
  call field_init
end subroutine

! nspecies, nx, nmode, nv, local allocation, deltaf, iptclshape, linear
subroutine ref_sizes(out) bind(C, name="ref_sizes")
  integer(c_int32_t), intent(out) :: out(8)
  out(1) = input_nspecies
  out(2) = input_nx
  out(3) = input_nmode
  out(4) = input_nv
  out(5) = particle_ip_high - particle_ip_low
  out(6) = input_deltaf
  out(7) = input_iptclshape
  out(8) = input_linear
end subroutine

subroutine ref_load() bind(C, name="ref_load")
  call particle_load
end subroutine

subroutine ref_compute_shape() bind(C, name="ref_compute_shape")
  call particle_compute_shape_x
end subroutine

subroutine ref_collect_charge() bind(C, name="ref_collect_charge")
  call interaction_collect_charge
end subroutine

subroutine ref_solve_field() bind(C, name="ref_solve_field")
  call field_solve_electric
end subroutine

subroutine ref_push(irk) bind(C, name="ref_push")
  integer(c_int), value :: irk
  global_irk = irk
  call interaction_push_particle
end subroutine

function ref_optimize(irk) result(did) bind(C, name="ref_optimize")
  integer(c_int), value :: irk
  integer(c_int) :: did
  logical :: flag
  global_irk = irk
  call particle_optimize(flag)
  did = merge(1, 0, flag)
end function

! particle_compute_dist_pertb_abs_v, then its result as [species][nv]
subroutine ref_dist_pertb_abs_v(out) bind(C, name="ref_dist_pertb_abs_v")
  real(c_double), intent(out) :: out(0 : input_nv - 1, input_nspecies)
  integer :: isp
  call particle_compute_dist_pertb_abs_v
  do isp = 1, input_nspecies
    out(:, isp) = particle_dist_pertb_abs_v(isp, :)
  end do
end subroutine

function marker_vec(isp, which) result(h)
  integer, intent(in) :: isp, which
  integer(kind=8) :: h
  select case (which)
  case (0)
    h = particle_x(isp)
  case (1)
    h = particle_v(isp)
  case (2)
    h = particle_p(isp)
  case (3)
    h = particle_w(isp)
  case (4)
    h = particle_x_bak(isp)
  case (5)
    h = particle_v_bak(isp)
  case default
    h = particle_w_bak(isp)
  end select
end function

subroutine ref_get_array(isp, which, out, n) bind(C, name="ref_get_array")
#include "finclude/petsc.h90"
  integer(c_int), value :: isp, which
  integer(c_int64_t), value :: n
  real(c_double), intent(out) :: out(n)
  real(kind=8), dimension(:), pointer :: a
  integer(kind=8) :: h
  h = marker_vec(isp + 1, which)
  call VecGetArrayF90(h, a, global_ierr)
  out(1 : n) = a(1 : n)
  call VecRestoreArrayF90(h, a, global_ierr)
end subroutine

subroutine ref_set_array(isp, which, in, n) bind(C, name="ref_set_array")
#include "finclude/petsc.h90"
  integer(c_int), value :: isp, which
  integer(c_int64_t), value :: n
  real(c_double), intent(in) :: in(n)
  real(kind=8), dimension(:), pointer :: a
  integer(kind=8) :: h
  h = marker_vec(isp + 1, which)
  call VecGetArrayF90(h, a, global_ierr)
  a(1 : n) = in(1 : n)
  call VecRestoreArrayF90(h, a, global_ierr)
end subroutine

function ref_get_np(isp) result(n) bind(C, name="ref_get_np")
  integer(c_int), value :: isp
  integer(c_int64_t) :: n
  n = particle_np(isp + 1)
end function

subroutine ref_set_np(isp, n) bind(C, name="ref_set_np")
  integer(c_int), value :: isp
  integer(c_int64_t), value :: n
  particle_np(isp + 1) = int(n, kind(particle_np))
end subroutine

function field_vec(which) result(h)
  integer, intent(in) :: which
  integer(kind=8) :: h
  select case (which)
  case (0)
    h = field_electric
  case (1)
    h = field_chargeden
  case (2)
    h = field_mode_re
  case (3)
    h = field_mode_im
  case default
    h = field_mode_grad_inv
  end select
end function

! which: 0 electric, 1 chargeden, 2 mode_re, 3 mode_im, 4 mode_grad_inv
subroutine ref_get_field(which, out, n) bind(C, name="ref_get_field")
#include "finclude/petsc.h90"
  integer(c_int), value :: which
  integer(c_int64_t), value :: n
  real(c_double), intent(out) :: out(n)
  real(kind=8), dimension(:), pointer :: a
  integer(kind=8) :: h
  h = field_vec(which)
  call VecGetArrayF90(h, a, global_ierr)
  out(1 : n) = a(1 : n)
  call VecRestoreArrayF90(h, a, global_ierr)
end subroutine

subroutine ref_set_field(which, in, n) bind(C, name="ref_set_field")
#include "finclude/petsc.h90"
  integer(c_int), value :: which
  integer(c_int64_t), value :: n
  real(c_double), intent(in) :: in(n)
  real(kind=8), dimension(:), pointer :: a
  integer(kind=8) :: h
  h = field_vec(which)
  call VecGetArrayF90(h, a, global_ierr)
  a(1 : n) = in(1 : n)
  call VecRestoreArrayF90(h, a, global_ierr)
end subroutine

! column imode of the cos (which = 0) or -sin (which = 1) matrix as field_init
! filled it: the product with a unit vector (0 + a * 1, every other term a * 0)
subroutine ref_field_table(which, imode, out) bind(C, name="ref_field_table")
#include "finclude/petsc.h90"
  integer(c_int), value :: which, imode
  real(c_double), intent(out) :: out(input_nx)
  real(kind=8), dimension(:), pointer :: a
  real(kind=8) :: keep(input_nmode)
  call VecGetArrayF90(field_mode_re, a, global_ierr)
  keep(:) = a(:)
  a(:) = 0.0_kpr
  a(imode + 1) = 1.0_kpr
  call VecRestoreArrayF90(field_mode_re, a, global_ierr)
  if (which == 0) then
    call MatMult(field_fourier_re, field_mode_re, field_tmp, global_ierr)
  else
    call MatMult(field_fourier_im, field_mode_re, field_tmp, global_ierr)
  end if
  call VecGetArrayF90(field_tmp, a, global_ierr)
  out(:) = a(:)
  call VecRestoreArrayF90(field_tmp, a, global_ierr)
  call VecGetArrayF90(field_mode_re, a, global_ierr)
  a(:) = keep(:)
  call VecRestoreArrayF90(field_mode_re, a, global_ierr)
end subroutine

subroutine ref_get_time(itime, time) bind(C, name="ref_get_time")
  integer(c_int32_t), intent(out) :: itime
  real(c_double), intent(out) :: time
  itime = global_itime
  time = global_time
end subroutine

subroutine ref_set_time(itime, time) bind(C, name="ref_set_time")
  integer(c_int32_t), value :: itime
  real(c_double), value :: time
  global_itime = itime
  global_time = time
end subroutine

! the driver's time update after the two sub-steps
subroutine ref_advance_time() bind(C, name="ref_advance_time")
  global_itime = global_itime + 1
  global_time = global_time + input_dt
end subroutine

! the indices of the next merge / remove / split event
subroutine ref_get_opt_index(out) bind(C, name="ref_get_opt_index")
  integer(c_int32_t), intent(out) :: out(3)
  out(1) = particle_imerge
  out(2) = particle_iremove
  out(3) = particle_isplit
end subroutine

subroutine ref_set_opt_index(in) bind(C, name="ref_set_opt_index")
  integer(c_int32_t), intent(in) :: in(3)
  particle_imerge = in(1)
  particle_iremove = in(2)
  particle_isplit = in(3)
end subroutine

! the spare value of the module's Gaussian pair: whether one is held, and which.
! A program run starts without one; within one process it outlives
! multirand_init, so `fresh` drops it where a stage stands for a new run.
subroutine ref_gaussian_spare(fresh, filled, spare) bind(C, name="ref_gaussian_spare")
  integer(c_int), value :: fresh
  integer(c_int32_t), intent(out) :: filled
  real(c_double), intent(out) :: spare
  if (fresh /= 0) multirand_gaussian64buf_filled = .false.
  filled = merge(1, 0, multirand_gaussian64buf_filled)
  spare = 0.0d0
  if (multirand_gaussian64buf_filled) spare = multirand_gaussian64buf
end subroutine

! the next n integers of the module's random stream (advances it)
subroutine ref_rng_ints(a, n) bind(C, name="ref_rng_ints")
  integer(c_int64_t), value :: n
  integer(c_int64_t), intent(out) :: a(n)
  call multirand_int_array64(a)
end subroutine

! the compiler's run-time exp, one call per element and as an array expression
subroutine ref_exp_array(x, y, n, vector) bind(C, name="ref_exp_array")
  integer(c_int64_t), value :: n
  integer(c_int), value :: vector
  real(c_double), intent(in) :: x(n)
  real(c_double), intent(out) :: y(n)
  integer(c_int64_t) :: i
  if (vector /= 0) then
    y(:) = exp(x(:))
  else
    do i = 1, n
      y(i) = exp(x(i))
    end do
  end if
end subroutine

! cos and sin of the same argument in one expression, as the loader forms them
subroutine ref_cos_sin_array(x, c, s, n) bind(C, name="ref_cos_sin_array")
  integer(c_int64_t), value :: n
  real(c_double), intent(in) :: x(n)
  real(c_double), intent(out) :: c(n), s(n)
  c(:) = cos(x(:))
  s(:) = sin(x(:))
end subroutine

end module ref_pic1dp_shim

"""Writes the input module the reference's hot-path sources are compiled against,
one per configuration of oracle/ref_cases.json (oracle/Makefile, target ref).

The reference's inputs are compile-time parameters of a module `pic1dp_input`;
this generator writes a module of that name holding the parameter names those
sources use, with the values of one case.  TEST INFRASTRUCTURE ONLY; its output
goes to oracle/_ref/<case>/ and is never committed.

  python gen_ref_input.py --list                 case names, one line
  python gen_ref_input.py --case NAME --out F    the module for one case
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402


def real(x):
    return "%s_kpr" % repr(float(x))


def reals(xs):
    xs = list(xs)
    if not xs:
        return "(/ real(kind = kpr) :: /)"
    return "(/ " + ", ".join(real(x) for x in xs) + " /)"


def ints(xs):
    xs = list(xs)
    if not xs:
        return "(/ integer(kind = kpi) :: /)"
    return "(/ " + ", ".join("%d" % int(x) for x in xs) + " /)"


def module_text(name):
    d = oracle.ref_case_values(name)
    ns, nm, ni = d["nspecies"], d["nmode"], d["init_nmode"]
    out = []
    add = out.append
    add("! written by oracle/gen_ref_input.py for case %s: do not edit" % name)
    add("module pic1dp_input")
    add("use pic1dp_global")
    add("implicit none")
    add('#include "finclude/petscdef.h"')
    for k in ("ntime_max", "linear", "iptcldist", "nspecies", "nmode", "init_nmode", "deltaf", "nparticle_max",
              "imarker", "nx", "nv", "iptclshape", "nmerge", "nremove", "nsplit", "typeremove", "split_ngroup",
              "multirand_al_int", "multirand_seed_type", "multirand_warmup", "nx_opd", "nv_opd"):
        add("PetscInt, parameter :: input_%s = %d" % (k, d[k]))
    add("PetscInt, parameter :: input_verbosity = 0")
    add("logical, parameter :: input_multirand_selftest = %s" % (".true." if d["multirand_selftest"] else ".false."))
    for k in ("time_max", "lx", "dt", "v_max", "remove_frac", "split_dv_sig_frac", "output_interval"):
        add("PetscReal, parameter :: input_%s = %s" % (k, real(d[k])))
    for k in ("charge", "mass", "temperature", "temperature2", "density", "v0"):
        add("PetscReal, dimension(input_nspecies), parameter :: input_species_%s = &" % k)
        add("  %s" % reals(d["species_" + k][:ns]))
    add("PetscInt, dimension(input_nspecies), parameter :: input_species_nparticle_init = &")
    add("  %s" % ints(d["species_nparticle_init"][:ns]))
    add("PetscInt, dimension(0 : input_nmode - 1), parameter :: input_modes = &")
    add("  %s" % ints(d["modes"][:nm]))
    add("PetscInt, dimension(0 : input_init_nmode - 1), parameter :: input_init_mode = &")
    add("  %s" % ints(d["init_mode"][:ni]))
    for k in ("init_mode_cos", "init_mode_sin"):
        add("PetscScalar, dimension(0 : input_init_nmode - 1), parameter :: input_%s = &" % k)
        add("  %s" % reals(d[k][:ni]))
    for kind in ("merge", "remove", "split"):
        n = d["n" + kind]
        for k in ("t" + kind, "thsh" + kind):
            add("PetscReal, dimension(input_n%s), parameter :: input_%s = &" % (kind, k))
            add("  %s" % reals(d[k][:n]))
    add("contains")
    add("! the perturbation's shape in velocity space: that of the markers")
    add("PetscScalar function input_pertb_shape(v, ispecies)")
    add("PetscScalar, intent(in) :: v")
    add("PetscInt, intent(in) :: ispecies")
    add("input_pertb_shape = 1.0_kpr")
    add("end function input_pertb_shape")
    add("end module pic1dp_input")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--case")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.list:
        print(" ".join(oracle.ref_case_names()))
        return
    text = module_text(a.case)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

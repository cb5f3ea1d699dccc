"""Restatement of the exact charge sum (kind 1, include/pic1dp_hip.h set_charge_sum) in numpy and Python ints: the cell
and left weight of every marker as the C oracle forms them (oracle/pic1dp_oracle.c orc_deposit_species_idx), every
contribution rounded once to whole quanta 2^e, hi / lo halves summed in int64, recombined in Python ints, converted
with float(int) (one rounding, to nearest even), then the FP64 steps of the library: species sum, nx/lx, -Z n0.
A helper of the tests, not collected."""
import math

import numpy as np

MASK32 = (1 << 32) - 1


def cells(x, inp):
    """wrapped positions, cell indices and left weights (src/pic1dp_interaction.F90:102-108)"""
    lx, nx = inp.lx, inp.nx
    px = np.fmod(np.asarray(x, dtype=np.float64), lx)
    px = np.where(px < 0.0, px + lx, px)
    sx = px / lx * float(nx)
    fl = np.floor(sx)
    wl = 1.0 - (sx - fl)
    ix = np.where((fl >= nx) | ~np.isfinite(fl), 0, fl).astype(np.int64)
    return px, ix, wl


def quantise(c, e):
    """n = rint(c 2^-e) (ties to even) as int64; c 2^-e is exact"""
    t = np.rint(np.asarray(c, dtype=np.float64) * np.ldexp(1.0, -e))
    assert np.all(np.abs(t) < 2.0 ** 62), "beyond the exact sum's range"
    return t.astype(np.int64)


def species_limbs(x, q, inp, e):
    """(hi, lo) per cell: the int64 sums of the contributions' high halves (signed) and low 32 bits"""
    nx = inp.nx
    _, ix, wl = cells(x, inp)
    q = np.asarray(q, dtype=np.float64)
    hi = np.zeros(nx, dtype=np.int64)
    lo = np.zeros(nx, dtype=np.int64)
    for cell, c in ((ix, wl * q), ((ix + 1) % nx, (1.0 - wl) * q)):   # :110, :113
        n = quantise(c, e)
        np.add.at(hi, cell, n >> 32)
        np.add.at(lo, cell, n & MASK32)
    return hi, lo


def totals(hi, lo):
    """hi 2^32 + lo per cell as Python ints"""
    return [(int(h) << 32) + int(v) for h, v in zip(hi, lo)]


def normalise(hi, lo):
    t = totals(hi, lo)
    return np.array([v >> 32 for v in t], dtype=np.int64), np.array([v & MASK32 for v in t], dtype=np.int64)


def rho_from_totals(t, e):
    q = 2.0 ** e
    return np.array([float(v) * q for v in t])


def exact_chargeden(xs, qs, inp, es):
    """xs, qs, es: per species.  Returns (chargeden, rho per species, totals per species)"""
    rhos, tots = [], []
    for x, q, e in zip(xs, qs, es):
        t = totals(*species_limbs(x, q, inp, e))
        tots.append(t)
        rhos.append(rho_from_totals(t, e))
    c2 = np.zeros(inp.nx)
    for s, rho in enumerate(rhos):           # charge_local_one's order
        c2 = c2 + rho * inp.species_charge[s]
    cd = c2 * float(inp.nx) / inp.lx
    if not inp.deltaf:
        for s in range(inp.nspecies):
            cd = cd - inp.species_charge[s] * inp.species_density[s]
    return cd, rhos, tots


def python_int_totals(x, q, inp, e):
    """the same totals by plain Python arithmetic, marker by marker (the self-check of the numpy path)"""
    nx, lx = inp.nx, inp.lx
    out = [0] * nx
    for xi, qi in zip(map(float, x), map(float, q)):
        px = math.fmod(xi, lx)
        if px < 0.0:
            px = px + lx
        sx = px / lx * float(nx)
        fl = math.floor(sx)
        wl = 1.0 - (sx - fl)
        ix = fl if fl < nx else 0
        for cell, c in ((ix, wl * qi), ((ix + 1) % nx, (1.0 - wl) * qi)):
            out[cell] += round(math.ldexp(c, -e))     # Python's round: ties to even
    return out

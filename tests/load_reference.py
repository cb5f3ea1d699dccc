"""The on-device particle load (include/pic1dp_hip.h pic1dp_hip_particle_load_device) restated: the index
function in numpy uint64 and Python integers, the marker values in np.longdouble.  No library call, no GPU."""
import numpy as np

M64 = (1 << 64) - 1
KEY_BASE = 0x7069633164704C44
GOLD = 0x9E3779B97F4A7C15
R3_DIGITS = 21
R3_SPAN = 3 ** 21
KNOWN_KEY = 1234567
KNOWN_DRAWS = (6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821)
PI = 3.14159265358979323846264   # PETSC_PI


def mix64_int(z):
    """the splitmix64 finaliser on a Python integer"""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def mix64(z):
    """... on a numpy uint64 array (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def key_of(seed_offset, ispecies):
    return mix64_int(KEY_BASE + 256 * seed_offset + ispecies)


def draws(key, c):
    """r(c) = mix64(key + (c + 1) GOLD) for a uint64 array of counters"""
    c = np.asarray(c, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix64(np.uint64(key) + (c + np.uint64(1)) * np.uint64(GOLD))


def bitrev64_int(g):
    return int(format(g & M64, "064b")[::-1], 2)


def r3_int(g):
    r = 0
    for _ in range(R3_DIGITS):
        r = r * 3 + g % 3
        g //= 3
    return r


def unit(r):
    """the top 53 bits of uint64 words as doubles in [0, 1)"""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def bitrev64(g):
    """the 64 bits of every word of a uint64 array reversed"""
    g = np.asarray(g, dtype=np.uint64).byteswap()        # bytes reversed; then the bits inside every byte
    for sh, mask in ((4, 0x0F0F0F0F0F0F0F0F), (2, 0x3333333333333333), (1, 0x5555555555555555)):
        g = ((g >> np.uint64(sh)) & np.uint64(mask)) | ((g & np.uint64(mask)) << np.uint64(sh))
    return g


def r3(g):
    """the 21 base-3 digits of every element of a uint64 array (below 3^21) reversed"""
    g = np.asarray(g, dtype=np.uint64).copy()
    r = np.zeros_like(g)
    for _ in range(R3_DIGITS):
        r = r * np.uint64(3) + g % np.uint64(3)
        g //= np.uint64(3)
    return r


def uniforms(kind, g, seed_offset=0, ispecies=0):
    """(u_v, u_x) of the global marker indices g (non-negative integers below 2^63)"""
    gg = np.array([int(v) for v in g] if not isinstance(g, np.ndarray) else g, dtype=np.uint64).reshape(-1)
    if kind == 1:
        key = key_of(seed_offset, ispecies)
        with np.errstate(over="ignore"):
            return unit(draws(key, np.uint64(2) * gg)), unit(draws(key, np.uint64(2) * gg + np.uint64(1)))
    assert kind == 2 and (gg.size == 0 or int(gg.max()) < R3_SPAN)
    uv = unit(bitrev64(gg))
    ux = r3(gg).astype(np.float64) / np.float64(R3_SPAN)   # both exact: one IEEE division
    return uv, ux


def block_np(inp, s, b, npe):
    spare = inp.nparticle_max - inp.species_nparticle_init[s]
    unload = spare // npe + (spare % npe if b == 0 else 0)
    return inp.nparticle_max // npe + (1 if inp.nparticle_max % npe > b else 0) - unload


def origin(inp, s, rank, nranks, npe):
    nblk = npe // nranks
    return sum(block_np(inp, s, b, npe) for b in range(rank * nblk))


def xv(inp, kind, s=0, g0=0, n=None, seed_offset=0):
    """x and v of global markers g0 ... g0 + n - 1 of species s: float64, bit for bit what the kernel stores"""
    n = inp.species_nparticle_init[s] if n is None else n
    uv, ux = uniforms(kind, np.arange(g0, g0 + n, dtype=np.uint64), seed_offset, s)
    return ux * np.float64(inp.lx), (uv - 0.5) * 2.0 * np.float64(inp.v_max)


def markers(inp, kind, s=0, g0=0, n=None, seed_offset=0):
    """x, v as xv() and p, w (np.longdouble, from those x and v: every operation of the formula in extended precision
    with libm's exp / sin / cos) of global markers g0 ... g0 + n - 1 of species s; beside them f (p before the perturbation), amp and every marker's
    largest |argument| of an exp, for the error bound"""
    x, v = xv(inp, kind, s, g0, n, seed_offset)
    n = x.size
    vmax, lx = np.float64(inp.v_max), np.float64(inp.lx)
    L = np.longdouble
    T, T2, m = L(inp.species_temperature[s]), L(inp.species_temperature2[s]), L(inp.species_mass[s])
    den, v0, ninit = L(inp.species_density[s]), L(inp.species_v0[s]), L(inp.species_nparticle_init[s])
    dist = inp.iptcldist
    pi = L(PI)
    pref = (L(1) if dist == 3 else den) * L(lx) * 2 * L(vmax) / ninit
    a1, a2 = 2 * T / m, 2 * T2 / m
    vl = v.astype(L)
    if dist == 1:
        q = vl * vl
        args = [q / 2]
        f = pref * q * np.exp(-q / 2) / np.sqrt(2 * pi)
    elif dist == 2:
        args = [(vl + v0) ** 2 / a1, (vl - v0) ** 2 / a1]
        f = pref * (np.exp(-args[0]) + np.exp(-args[1])) / np.sqrt(8 * pi * T / m)
    elif dist == 3:
        args = [vl * vl / a1, (vl - v0) ** 2 / a2]
        f = pref * (den * np.exp(-args[0]) / np.sqrt(2 * pi * T / m) + (1 - den) * np.exp(-args[1]) / np.sqrt(2 * pi * T2 / m))
    else:
        args = [(vl - v0) ** 2 / a1]
        f = pref * np.exp(-args[0]) / np.sqrt(2 * pi * T / m)
    amp = np.zeros(n, dtype=L)
    for j in range(inp.init_nmode):
        kk = L(np.float64(2.0 * PI / inp.lx * float(inp.init_mode[j])))   # the host's constant, a double
        arg = (np.float64(kk) * x).astype(L)                              # the kernel's argument, a rounded double
        amp = amp + L(inp.init_mode_cos[j]) * np.cos(arg) + L(inp.init_mode_sin[j]) * np.sin(arg)
    w = amp * f
    p = f + w if inp.linear == 0 else f
    return dict(x=x, v=v, p=p, w=w, f=f, amp=amp, arg=np.maximum.reduce(args))

"""Random call sequences for the differential of the on-demand marker products and the restart (DESIGN.md 0;
tests/test_gpu_call_sequences.py runs them, tests/test_call_sequences_host.py counts what they cover).  A pure generator:
sequence(seed, mode) uses no GPU and reads no engine's output.  A helper of the tests, not collected.

The skeleton is the reference's sequence push(1), collect_charge, solve_field, push(2), collect_charge, solve_field.  An
intruder is a call between two of them; WHERE is named by the boundary: B0 between time steps, B1 ... B5 after the first ...
fifth call, P between charge_local and charge_reduced (their _exact pair in mode `exact`) of a split-phase deposit
(`hostsum`, itself an intruder at any boundary).

Two kinds of intruder.  READ_ONLY are the calls that promise to cache nothing and change nothing: the products, the digest,
output_all and the checkpoint -- at B0, between time steps, a write followed by a restart of the run from the file
(expect "restart"), inside a time step and at P a write that has to be refused (expect "refused").  STATE_CHANGING are the
ones the older single-call differential (tests/test_gpu_fuzz.py _single_calls) already knew, kept so that the products meet
the states they create.

Legality is tracked by a small model of what the calls leave behind: the cursor in the six calls, whether push(2) has an RK
backup to read, the solver and transform switches, a split deposit pending, and the library's own record of where the host
stands in a time step (call_phase: pic1dp_hip_checkpoint_write refuses unless it is 0).

So that few seeds cover everything, every (read-only intruder, boundary) pair is a card of a deck that is shuffled and dealt
over the DEFAULT_SEEDS[mode] seeds of a block (seeds b n ... b n + n - 1); on top of its cards a seed draws intruders at
random.  One card of every kind is flagged: another read-only intruder follows it directly (the products share one device
buffer and the pinned staging)."""
import numpy as np

MODES = ("tiles", "sums", "exact")
KIND = {"tiles": 1, "sums": 2, "exact": 0}     # PIC1DP_PRED_KIND of engines a and c (0: left alone -- the exact charge sum predicts nothing)
NOPS = 80                                      # calls per seed, intruders and the quiet stretches of `sums` included
# Two needs set the number of default seeds of a mode, and the larger one is what the suite runs (the census of
# tests/test_call_sequences_host.py holds both, and that no smaller number serves):
#   - A seed plays at most one card in five calls, so that the reference's own sequence keeps the larger share of a seed and
#     a card mostly meets a state that random calls, not other cards, have made.  The deck has 71 cards (_deck):
#     ceil(71 / 16) = 5 seeds.
#   - Every (kind, place) pair of the four kinds whose references sum with math.fsum or in Python integers is held against
#     that reference at least once (referenced()): 28 pairs, at most MAX_REFERENCES evaluations per seed, one per intrusion
#     with the exact sums and two otherwise: ceil(28 / 8) = 4 seeds in `exact`, ceil(28 / 4) = 7 in `tiles` and `sums`.
MAX_CARDS = NOPS // 5
NCARDS = 71
REFERENCED = ("moments", "moments_local_exact", "power", "power_local_exact")
MAX_REFERENCES = 8      # evaluations of those references per seed


def reference_quota(mode):
    """intrusions per seed that get the reference: one evaluation each with the exact sums (b's markers serve a too), two
    otherwise (a's own download and b's)"""
    return MAX_REFERENCES // (1 if mode == "exact" else 2)


def seeds_needed(mode):
    return max(-(-NCARDS // MAX_CARDS), -(-len(REFERENCED) * 7 // reference_quota(mode)))


DEFAULT_SEEDS = {mode: seeds_needed(mode) for mode in MODES}

REF = ("push1", "collect", "solve", "push2", "collect", "solve")
PLACES = ("B0", "B1", "B2", "B3", "B4", "B5", "P")
READ_ONLY = ("moments", "moments_local_exact", "power", "power_local_exact", "select", "select_count", "gather", "state_digest",
             "output_all", "checkpoint")
STATE_CHANGING = ("step", "substep1", "substep2", "setE", "setcd", "solver", "transform", "optimize", "upload", "download")


class Model:
    """what the calls so far leave behind, as far as legality needs it"""

    def __init__(self):
        self.cursor, self.rk_ok, self.fd, self.tr, self.phase = 0, False, 0, 0, 0

    def place(self):
        return "B%d" % self.cursor

    def collected(self):
        if self.phase in (1, 4):
            self.phase += 1

    def ref(self, op):
        if op == "push1":
            self.rk_ok, self.phase = True, 1
        elif op == "push2":
            self.rk_ok, self.phase = False, 4
        elif op == "collect":
            self.collected()
        elif self.phase == 2:
            self.phase = 3
        elif self.phase == 5:
            self.phase = 0
        self.cursor = (self.cursor + 1) % 6

    def intruder(self, op):
        if op == "step":
            self.rk_ok, self.phase = False, 0
        elif op == "substep1":
            self.rk_ok, self.phase = True, 3
        elif op == "substep2":
            self.rk_ok, self.phase = False, 0
        elif op == "optimize":
            self.rk_ok = False
        elif op == "upload":
            self.rk_ok, self.phase = False, 0
        elif op == "hostsum":
            self.collected()


def _inputs(rng, seed, mode):
    """input keywords as _single_calls draws them, with an odd nparticle_max, the output grid, two species and npe by seed"""
    kind = KIND[mode]
    nx = int(rng.choice([32, 48, 64, 96, 100]))
    nmode = 1 if (mode == "sums" and rng.random() < 0.75) else int(rng.choice([1, 2]))
    modes = [1] if nmode == 1 else sorted(rng.choice(np.arange(1, nx // 2), size=2, replace=False).tolist())
    nmax = 20001 + 2 * int(rng.integers(0, 5001))
    nxo, nvo = ((8, 8), (16, 32))[int(rng.integers(0, 2))]
    dist = int(rng.choice([0, 2, 3, 3]))
    two = seed % 5 in (1, 3)
    npe = 2 if seed % 5 in (0, 3) else 1
    nsp = 2 if two else 1
    kw = dict(nparticle_max=nmax, nx=nx, nmode=nmode, modes=[int(m) for m in modes], iptcldist=dist,
              linear=int(rng.random() < 0.25), init_nmode=nmode, init_mode=[int(m) for m in modes],
              init_mode_sin=[1e-3] * nmode, init_mode_cos=[0.0] * nmode, nx_opd=nxo, nv_opd=nvo)
    nonpow2 = rng.random() < 0.3
    if two:
        kw.update(nspecies=2, species_nparticle_init=[nmax, 7001], species_charge=[-1.0, 1.0],
                  species_mass=[1.1, 3.7] if nonpow2 else [1.0, 4.0],
                  species_temperature=[1.3, 0.9] if nonpow2 else [1.0, 1.0],
                  species_temperature2=[0.7, 1.1] if nonpow2 else [1.0, 1.0],
                  species_density=[1.0, 0.8] if dist == 2 else [0.9, 0.75],
                  species_v0=[3.0, 2.5] if dist == 2 else [5.0, 4.0])
    else:
        if dist == 2:
            kw.update(species_density=[1.0], species_v0=[3.0])
        if nonpow2:
            kw.update(species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1])
    load = "device" if seed % 4 == 2 else "host"
    return kw, npe, nsp, load, kind == 2 and mode == "sums" and nmode == 1


def _deck(mode, block):
    """the block's cards (kind, place, follow), shuffled: every pair once, the restart at B0 twice"""
    rng = np.random.default_rng([4021, MODES.index(mode), block])
    cards = [[k, p, False] for k in READ_ONLY for p in PLACES] + [["checkpoint", "B0", False]]
    for k in READ_ONLY:
        mine = [c for c in cards if c[0] == k]
        mine[int(rng.integers(0, len(mine)))][2] = True
    assert len(cards) == NCARDS
    order = rng.permutation(len(cards))
    return [tuple(cards[i]) for i in order]


def _read_only_args(rng, kind, kw, nsp):
    isp = int(rng.integers(0, nsp))
    if kind in ("moments", "moments_local_exact", "power", "power_local_exact"):
        return dict(isp=isp, which=int(rng.integers(1, 4)))
    if kind in ("select", "select_count"):
        lo, hi = float(rng.random()), float(rng.random())       # fractions of lx; lo > hi crosses the periodic end
        v_lo = float(rng.uniform(-5.0, 3.0))
        return dict(isp=isp, x=(lo, hi), v=(v_lo, v_lo + float(rng.uniform(0.5, 6.0))),
                    fraction=float(rng.choice([1.0, 0.5, 1.0 / 16.0])), key=int(rng.integers(0, 1000)))
    if kind == "gather":
        nalloc = kw["nparticle_max"]                            # one context: every species owns nparticle_max slots
        npv = kw["species_nparticle_init"][isp] if "species_nparticle_init" in kw else nalloc
        idx = rng.integers(0, nalloc, size=int(rng.integers(1, 48))).tolist()
        idx += idx[:3] + [0, npv - 1, nalloc - 1]               # duplicates, the last valid marker, the last slot
        if npv < nalloc:
            idx += [npv, int(rng.integers(npv, nalloc))]        # tail slots
        return dict(isp=isp, index=[int(i) for i in rng.permutation(idx)])
    return {}


def sequence(seed, mode):
    """dict(kw, npe, nspecies, load, pair_case, ops): ops is a list of (op, args); the args of an intruder carry `at`, its
    boundary, a read-only one also `after_quiet` (2 or 3: it is the call right behind a quiet push1, collect / its solve of
    the pair path) where that holds; `hostsum` carries `inside`, the read-only intruders at P"""
    assert mode in MODES
    rng = np.random.default_rng([977, MODES.index(mode), seed])
    kw, npe, nsp, load, pair_case = _inputs(rng, seed, mode)
    n = DEFAULT_SEEDS[mode]
    cards = [c for j, c in enumerate(_deck(mode, seed // n)) if j % n == seed % n]
    assert len(cards) <= MAX_CARDS
    # a card is not played before `due` calls have gone: the cards spread over the first two thirds of the sequence
    hand = sorted(((int(rng.integers(0, 2 * NOPS // 3)), c) for c in cards), key=lambda t: t[0])
    m, ops = Model(), []
    plan = sorted(rng.choice(np.arange(2, NOPS - 30), size=2, replace=False).tolist()) if pair_case else []
    setups, quiet, forced = [14, 15], 0, 0

    def read_only(kind, at, **extra):
        args = _read_only_args(rng, kind, kw, nsp)
        if kind == "checkpoint":
            args["expect"] = "restart" if (at == "B0" and m.phase == 0) else "refused"
            if args["expect"] == "restart":
                m.rk_ok = False                                 # (the file carries no RK backup)
        args.update(at=at, **extra)
        return (kind, args)

    def playable(kind, at):
        """a checkpoint is dealt only where the model knows what it does: the restart at B0 with call_phase 0, the refusal
        with call_phase != 0 or at P"""
        if kind != "checkpoint" or at == "P":
            return True
        return m.phase != 0 or at == "B0"

    def due_card(at, count):
        for i, (due, c) in enumerate(hand):
            if due > count or c[1] != at or not playable(c[0], at):
                continue
            if c[0] == "checkpoint" and at == "B0" and m.phase != 0:    # (the card at B0 is the restart)
                continue
            return hand.pop(i)[1]
        return None

    def random_read_only(at):
        while True:
            kind = str(rng.choice(READ_ONLY))
            if playable(kind, at):
                return kind

    def run_of_read_only(first, at, follow, **extra):
        """a read-only intruder and, flagged or by chance, more of them directly behind it"""
        out = [read_only(first, at, **extra)]
        while follow or rng.random() < 0.25:
            follow = False
            out.append(read_only(random_read_only(at), at))
        return out

    count = 0
    while count < NOPS or (hand and count < 2 * NOPS):    # (a hand not yet played out: a few calls more)
        count += 1
        if plan and count >= plan[0] and m.cursor == 0 and quiet == 0 and not forced:
            plan.pop(0)
            quiet = setups.pop(0)
            m.fd = m.tr = 0
            ops.append(("pair-setup", {}))
        at = m.place()
        card = None if (quiet or forced) else due_card(at, count)
        p_card = None if (quiet or forced or card) else due_card("P", count)
        if forced:                                              # right behind the quiet stretch: a read-only intruder
            c = due_card(at, 3 * NOPS)
            first, follow = (c[0], c[2]) if c else (random_read_only(at), False)
            ops.extend(run_of_read_only(first, at, follow, after_quiet=forced))
            forced = 0
            continue
        if card:
            ops.extend(run_of_read_only(card[0], at, card[2]))
            continue
        if p_card or (quiet == 0 and rng.random() < 0.06):      # a split-phase deposit with intruders inside
            first, follow = (p_card[0], p_card[2]) if p_card else (random_read_only("P"), False)
            ops.append(("hostsum", dict(at=at, inside=run_of_read_only(first, "P", follow))))
            m.intruder("hostsum")
            continue
        if quiet == 0 and rng.random() < 0.3:
            if rng.random() < 0.4:
                ops.extend(run_of_read_only(random_read_only(at), at, False))
                continue
            op = str(rng.choice(STATE_CHANGING + ("hostsum",)))
            if op == "substep2" and not m.rk_ok:
                op = "substep1"
            args = dict(at=at)
            if op == "step":
                args["n"] = int(rng.integers(1, 3))
            elif op == "setE":
                args.update(phase=float(rng.random()), noise=int(rng.integers(0, 2**31)))
            elif op == "setcd":
                args["factor"] = 1.0 + 0.25 * float(rng.random())
            elif op == "solver":
                m.fd = args["kind"] = 1 - m.fd
            elif op == "transform":
                m.tr = args["kind"] = 1 - m.tr
            elif op == "hostsum":
                args["inside"] = []
            m.intruder(op)
            ops.append((op, args))
            continue
        op = REF[m.cursor]
        if op == "push2" and not m.rk_ok:                       # push(2) reads the RK backup: only behind a push(1) / substep(1)
            m.cursor, op = 0, "push1"
        ops.append((op, {}))
        m.ref(op)
        if quiet:
            quiet -= 1
            if quiet == 0:
                forced = m.cursor                               # 2: behind push1, collect; 3: behind its solve
    assert not hand, ("cards left over", mode, seed, hand)
    return dict(kw=kw, npe=npe, nspecies=nsp, load=load, pair_case=pair_case, ops=ops)


def intrusions(seq):
    """[(kind, place, args, next)] of the read-only intruders of a sequence in order, those inside a hostsum included;
    `next` is the op that follows directly (inside a hostsum: the next one inside, or "charge_reduced")"""
    out = []
    ops = seq["ops"]
    for i, (op, args) in enumerate(ops):
        nxt = ops[i + 1][0] if i + 1 < len(ops) else "end"
        if op in READ_ONLY:
            out.append((op, args["at"], args, nxt))
        elif op == "hostsum":
            inside = args["inside"]
            for j, (k, a) in enumerate(inside):
                out.append((k, "P", a, inside[j + 1][0] if j + 1 < len(inside) else "charge_reduced"))
    return out


def without_read_only(ops):
    """the sequence engine c runs: the read-only intruders removed, a split deposit unsplit"""
    out = []
    for op, args in ops:
        if op in READ_ONLY:
            continue
        out.append((op, dict(args, inside=[]) if op == "hostsum" else args))
    return out


# -- which intrusions are held against the expensive references -----------------------------------------------------------
_REFERENCED_CACHE = {}


def referenced(seed, mode):
    """the ordinals (positions in intrusions(sequence(seed, mode))) of the intrusions of this seed that are held against
    the fsum / Python-integer references.  Chosen for the whole block of seeds at once, by (kind, place): every pair of a
    REFERENCED kind and a place is referenced in at least one seed of the block (a matching of the 28 pairs to the seeds'
    quotas; None for a pair no seed has room for -- the census fails then); what is left of a seed's quota goes to its
    first intrusions of those kinds not yet taken."""
    n = DEFAULT_SEEDS[mode]
    block = seed // n
    if (mode, block) not in _REFERENCED_CACHE:
        quota = reference_quota(mode)
        seeds = list(range(block * n, block * n + n))
        where = {}                              # (kind, place) -> {seed: first ordinal}
        for s in seeds:
            for i, (kind, place, _, _) in enumerate(intrusions(sequence(s, mode))):
                if kind in REFERENCED:
                    where.setdefault((kind, place), {}).setdefault(s, i)
        taken = {s: {} for s in seeds}          # seed -> {pair: ordinal}

        def assign(pair, visited):              # augmenting path: a seed with room, or one whose pair can move
            for s in where.get(pair, {}):
                if s in visited:
                    continue
                visited.add(s)
                if len(taken[s]) < quota:
                    taken[s][pair] = where[pair][s]
                    return True
                for other in list(taken[s]):
                    if assign_moved(other, s, visited):
                        taken[s][pair] = where[pair][s]
                        return True
            return False

        def assign_moved(pair, away_from, visited):
            del taken[away_from][pair]
            if assign(pair, visited):
                return True
            taken[away_from][pair] = where[pair][away_from]
            return False

        missing = [(k, p) for k in REFERENCED for p in PLACES if not assign((k, p), set())]
        chosen = {}
        for s in seeds:
            mine = set(taken[s].values())
            for i, (kind, _, _, _) in enumerate(intrusions(sequence(s, mode))):
                if len(mine) >= quota:
                    break
                if kind in REFERENCED:
                    mine.add(i)
            chosen[s] = mine
        _REFERENCED_CACHE[(mode, block)] = (chosen, missing)
    chosen, missing = _REFERENCED_CACHE[(mode, block)]
    return chosen[seed], missing

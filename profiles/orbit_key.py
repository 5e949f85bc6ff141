"""Python restatement of csrc/orbit_key.hpp (the orbit of a tile in the XCD-aware processing order), used by the L2 model
(profiles/l2_model.py) and compared with the C++ function for every prefix by tests/test_orbit_key_host.py.

orbit_key(P, p, quad_blocks, cap_tenths) -> (representative, member id, moves); moves lists what the orbit may change:
("quad", b, k): sites b..b+3 take any configuration with k up spins; ("pair", b): sites b, b+1 (one up, one down) swap."""

QUAD_COUNT = (1, 4, 6, 4, 1)
QUAD_MBITS = (0, 2000, 2585, 2000, 0)          # log2 of the count in thousandths of a bit, rounded up


def orbit_key(P, p, quad_blocks, cap_tenths):
    cap = 100 * cap_tenths
    rep, member, mult, used, moves = P, 0, 1, 0, []
    b = 1
    while b + 1 <= p:
        if b % 4 == 1 and (b - 1) // 4 < quad_blocks and b + 3 <= p:
            cfg = (P >> (b - 1)) & 15
            k = bin(cfg).count("1")
            if QUAD_COUNT[k] > 1 and used + QUAD_MBITS[k] <= cap:
                digit = sum(1 for c in range(cfg) if bin(c).count("1") == k)
                rep = (rep & ~(15 << (b - 1))) | (((1 << k) - 1) << (b - 1))
                member += digit * mult
                mult *= QUAD_COUNT[k]
                used += QUAD_MBITS[k]
                moves.append(("quad", b, k))
                b += 4
                continue
        if ((P >> (b - 1)) ^ (P >> b)) & 1 and used + 1000 <= cap:
            if not (P >> (b - 1)) & 1:
                rep ^= 3 << (b - 1)
                member += mult
            mult *= 2
            used += 1000
            moves.append(("pair", b))
        b += 2
    return rep, member, moves


def neighbours(P, moves):
    """every prefix one move away from P"""
    out = []
    for mv in moves:
        if mv[0] == "pair":
            out.append(P ^ (3 << (mv[1] - 1)))
        else:
            _, b, k = mv
            cur = (P >> (b - 1)) & 15
            out.extend((P & ~(15 << (b - 1))) | (c << (b - 1)) for c in range(16) if bin(c).count("1") == k and c != cur)
    return out


# ---- restatement of csrc/xcd_deal.hpp: the costs of a tile and the dealing of orbits to the eight XCD queues ----
from math import comb  # noqa: E402

DEAL_COSTS = ("rr", "rows", "slots", "req", "out")           # sd_deal_cost 0..4; a mix is (w_a, cost_a, w_b, cost_b)


def tile_costs(P, p, LS, nup, quad_blocks, cap_tenths):
    """(rows, slots, requested bytes, out-of-orbit bytes) of tile P.  A partner across a flippable prefix bond (b, b+1) is a
    member of P's orbit exactly when the bond is a generator pair or lies inside a quad-active block (every other flip changes
    the filling of a unit, which the representative keeps)."""
    t = nup - bin(P).count("1")
    ln = comb(LS, t) if 0 <= t <= LS else 0
    if (P >> (p - 1)) & 1:
        straddle = comb(LS - 1, t) if 0 <= t <= LS - 1 else 0
    else:
        straddle = comb(LS - 1, t - 1) if 1 <= t <= LS else 0
    _, _, moves = orbit_key(P, p, quad_blocks, cap_tenths)
    closed = set()
    for mv in moves:
        closed.update((mv[1],) if mv[0] == "pair" else (mv[1], mv[1] + 1, mv[1] + 2))
    partners = inside = 0
    for b in range(1, p):
        if ((P >> (b - 1)) ^ (P >> b)) & 1:
            partners += 1
            inside += b in closed
    req = 16 * ((2 + partners) * ln + straddle)
    return ln, (ln + 255) // 256, req, req - 16 * inside * ln


def parse_cost(name):
    """'rows' -> 'rows'; 'mix:3:rows:40:slots' -> (3, 'rows', 40, 'slots')   (a trailing ':run<n>' is the caller's to strip)"""
    if name.startswith("mix:"):
        _, wa, ca, wb, cb = name.split(":")
        return int(wa), ca, int(wb), cb
    if name not in DEAL_COSTS:
        raise ValueError("unknown dealing cost " + name)
    return name


def cost_of(orbit, cost):
    """orbit = (tiles, rows, slots, req, out) summed over its tiles"""
    if isinstance(cost, tuple):
        wa, ca, wb, cb = cost
        return wa * orbit[DEAL_COSTS.index(ca)] + wb * orbit[DEAL_COSTS.index(cb)]
    return 0 if cost == "rr" else orbit[DEAL_COSTS.index(cost)]


def deal(orbits, cost, run=1):
    """queue index per orbit, in sequence order: a run of `run` consecutive orbits goes to the queue with the lowest cost so far,
    ties to the lowest index; 'rr': run number % 8"""
    q_cost, out, x = [0] * 8, [], 0
    for o, orb in enumerate(orbits):
        if o % run == 0:
            x = (o // run) % 8 if cost == "rr" else q_cost.index(min(q_cost))
        q_cost[x] += cost_of(orb, cost)
        out.append(x)
    return out

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

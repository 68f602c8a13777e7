"""How many register links a deal of the diagonals of BCH(255,231) can have.  A link is a compile-time slot pair of the
kernel (minsum_diag_impl.hpp, CHAIN): all 16 lanes of a frame need one in the same slots, so L links per lane need 16 L
disjoint pairs of diagonals (s, s + g), consecutive in the support so that the column's summation order holds.  Prints
the maximal runs of consecutive diagonals, the largest sets of disjoint gap-1 pairs and of disjoint triples, and, with
32 disjoint gap-1 pairs taken (the two links per lane the kernel has), the most disjoint consecutive gap-g pairs that
remain for a third link, g = 1 .. 4.  DESIGN.md 8 item 2, profiles/r25_experiments.md."""
from deal_model import SUPPORT_255_231


def runs(sup):
    out, cur = [], [sup[0]]
    for a, b in zip(sup, sup[1:]):
        if b == a + 1:
            cur.append(b)
        else:
            out.append(cur)
            cur = [b]
    return out + [cur]


def third_link_pairs(sup, g, need=32):
    """Most disjoint pairs of neighbours in the support that are g apart, next to `need` disjoint pairs 1 apart.  The
    candidate pairs join neighbours of the sorted support, so this is a matching on a path: best[k][a] = most gap-g pairs
    among the first k diagonals with a gap-1 pairs taken (a capped at need)."""
    NEG = -10 ** 9
    cap = lambda a: min(a, need)
    best = [[NEG] * (need + 1) for _ in range(len(sup) + 1)]
    best[0][0] = 0
    for k in range(len(sup)):
        for a in range(need + 1):
            v = best[k][a]
            if v == NEG:
                continue
            best[k + 1][a] = max(best[k + 1][a], v)  # diagonal k stays single (or was paired with k - 1)
            if k + 1 < len(sup):
                gap = sup[k + 1] - sup[k]
                if gap == 1:
                    best[k + 2][cap(a + 1)] = max(best[k + 2][cap(a + 1)], v)
                if gap == g:
                    best[k + 2][a] = max(best[k + 2][a], v + 1)
    return best[len(sup)][need]


if __name__ == "__main__":
    sup = SUPPORT_255_231
    rs = runs(sup)
    table = {}
    for r in rs:
        table[len(r)] = table.get(len(r), 0) + 1
    print("support", len(sup), "diagonals; runs of consecutive diagonals (length: count):", dict(sorted(table.items())))
    print("disjoint gap-1 pairs:", sum(len(r) // 2 for r in rs), "(three links per lane need 48)")
    print("disjoint triples:", sum(len(r) // 3 for r in rs), "(a three-diagonal chain per lane needs 16)")
    for g in (1, 2, 3, 4):
        print("gap-%d pairs next to 32 gap-1 pairs:" % g, third_link_pairs(sup, g), "(a third link needs 16)")

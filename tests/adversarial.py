"""Random small networks with every outcome (Optimal / Infeasible / Unbounded), shared by the single-solve engine's and the batch solver's
fuzz tests: lower bounds, infinite and zero capacities, negative and 64-bit costs, ties, self loops, parallel arcs, unbalanced supplies."""
import numpy as np

from oracle import ns_oracle as O


def random_problem(rng, n, m, supply_kind, *, cost_scale=1, ties=False, zero_capacity=True, inf_fraction=0.1, bound_infeasible=False):
    """supply_kind: "balanced" / "negative" (costs from -6) / "excess" (3 units too many).  The defaults are the generator of
    test_random_small_networks_all_outcomes, draw for draw; every keyword draws more (or otherwise) only when it leaves its default.
      cost_scale        costs are multiplied by it and get a jitter in [-3, 3]: the order of reduced costs is decided in the high bits, with
                        near-ties that only the low bits settle
      ties              costs are replaced by their sign: -1 / 0 / 1
      zero_capacity     whether upper == lower may be drawn (the C# semantics answers Unbounded on an eligible arc of capacity 0 that nothing
                        blocks, so with many arcs and zero capacities allowed nearly every instance ends there)
      inf_fraction      share of uncapacitated arcs
      bound_infeasible  one arc gets upper < lower: Infeasible before the first pivot"""
    src = rng.integers(0, n, m).astype(np.int32)
    tgt = rng.integers(0, n, m).astype(np.int32)
    lower = np.where(rng.random(m) < 0.15, rng.integers(0, 4, m), 0).astype(np.int64)
    upper = (lower + rng.integers(0 if zero_capacity else 1, 12, m)).astype(np.int64)
    upper[rng.random(m) < inf_fraction] = O.INF_CAP
    cost = rng.integers(-6 if supply_kind == "negative" else 0, 20, m).astype(np.int64)
    if ties:
        cost = np.sign(cost)
    if cost_scale != 1:
        cost = cost * np.int64(cost_scale) + rng.integers(-3, 4, m)
    supply = np.zeros(n, np.int64)
    k = max(1, n // 4)
    s = rng.integers(1, 9, k)
    supply[rng.choice(n, k, replace=False)] += s
    supply[rng.choice(n, k, replace=False)] -= rng.permutation(s)
    if supply_kind == "excess":
        supply[rng.integers(0, n)] += 3          # unbalanced: whatever the C# solver makes of it, both sides must agree
    if bound_infeasible:
        e = int(rng.integers(0, m))
        upper[e] = lower[e] - 1
    return O.Problem(n, m, src, tgt, lower, upper, cost, supply)


# m + n = the range the three rules stride by the 64 lanes of a wave: one short of, at and one past every multiple up to four strides,
# ten strides exactly, and a size that is no multiple
SEARCH_ARCS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 640, 1000)
PER_SIZE = 24
BIG_COST = 1 << 40        # with n <= 60: |cost| < 2^45, art_cost = (max |cost| + 1) n < 2^51, potentials and reduced costs far inside int64
SEED = 20261017


def adversarial_batch():
    """[(problem, supply type)]: 24 instances for every size of SEARCH_ARCS, n in [1, min(m + n, 60)].  By the running index k:
    kind balanced / negative / excess (k % 3); costs plain / ties / BIG_COST / plain (k % 4); LEQ every fifth; zero capacities allowed
    every 11th (coprime to 3, 4 and 5, so they meet every kind and cost mode); one arc infeasible by its bounds every 67th.
    Uncapacitated arcs: 0.1 of them, but none in seven of eight negative-cost instances and in none above 257 search arcs.  The C# semantics
    answers an uncapacitated negative cycle Optimal with flows at its infinity constant and a total cost that wraps; the fuzz asserts that
    the reference's numbers did not overflow, and a dense graph of at most 60 nodes nearly always holds such a cycle (34 of 40 random
    instances at 1000 search arcs, 22 of 40 at 640, 2 of 9 at 65)."""
    rng = np.random.default_rng(SEED)
    out = []
    for size in SEARCH_ARCS:
        for _ in range(PER_SIZE):
            k = len(out)
            n = int(rng.integers(1, min(size, 60) + 1))
            m = size - n
            kind = ("balanced", "negative", "excess")[k % 3]
            mode = k % 4
            inf_fraction = 0.0 if kind == "negative" and ((k // 3) % 8 != 0 or size > 257) else 0.1
            p = random_problem(rng, n, m, kind, cost_scale=BIG_COST if mode == 2 else 1, ties=mode == 1, zero_capacity=k % 11 == 5,
                               inf_fraction=inf_fraction, bound_infeasible=m > 0 and k % 67 == 40)
            out.append((p, O.LEQ if k % 5 == 4 else O.GEQ))
    return out

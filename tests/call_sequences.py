"""A model of the calls one long-lived sa_context (DeviceBuilder) serves, and
a deterministic order of them that covers every ordered pair.

TEST INFRASTRUCTURE ONLY: the model chooses inputs (which call follows which);
it computes no expected value.  tests/test_call_sequences.py asserts its
properties on the CPU, tests/test_gpu_call_sequences.py runs the walk on one
context and compares every step with a reference of the operation itself.

A context carries state from call to call (the radix tile states and their
epoch, the radix algorithm, the alphabet flags, the member bitmap, the lazily
allocated group-start buffers, cursors, error words, the pinned read-back
words, capacities that grow by reallocation), so what a call leaves behind
matters to whichever call comes next.  The walk is an Eulerian circuit of the
complete directed graph with loops over the operations: K * K edges, K * K + 1
nodes, every ordered pair (a -> b), a == b included, exactly once.
"""

# build variants: name -> keyword arguments of DeviceBuilder.build.  The
# degenerate and periodic variants differ by their text, not by an option.
BUILD_VARIANTS = {
    "build_default": {},
    "build_reference": {"schedule": "reference"},
    "build_lsd": {"round1": "lsd"},
    "build_bucketed": {"round1": "bucketed"},
    "build_reduce_scan": {"radix": "reduce_scan"},
    "build_perm_always": {"schedule": "reference", "debug": ("perm_always",)},
    "build_alpha_sample_small": {"round1": "bucketed", "debug": ("alpha_sample_small",)},
    "build_degenerate": {},
    "build_periodic": {},
}

OPERATIONS = tuple(BUILD_VARIANTS) + (
    "check_valid",          # verdict True
    "check_swapped",        # two adjacent entries swapped: verdict False
    "lcp_valid",
    "lcp_duplicate",        # SAError
    "inverse_valid",
    "inverse_duplicate",    # SAError
    "locate",
    "mems",
    "lpf_lz77",
    "repeats",
    "lf_ibwt",
    "fm_build_locate",
    "argsort",
    "pack_keys",
    "generate_text",
)


def eulerian_walk(k: int) -> list:
    """Node indices of a closed walk from node 0 over the complete digraph
    with loops on k nodes that uses each of the k * k edges once (Hierholzer;
    out-edges are taken in ascending order of their head, so two calls agree)."""
    if k < 1:
        raise ValueError("k must be at least 1")
    nxt = [0] * k                 # the next unused out-edge of each node: v -> nxt[v]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            stack.append(nxt[v])
            nxt[v] += 1
        else:
            walk.append(stack.pop())
    walk.reverse()
    return walk


def walk(ops=OPERATIONS) -> list:
    """The operations' names in the order of eulerian_walk(len(ops))."""
    return [ops[i] for i in eulerian_walk(len(ops))]


def pairs(seq) -> list:
    """The ordered pairs (previous, this) of a sequence of steps."""
    return list(zip(seq[:-1], seq[1:]))


# ---- the epoch of the radix tile states ------------------------------------
# A context tags its tile states with an epoch of EPOCH_BITS bits, one per
# radix pass; the pass that would take tag 2^EPOCH_BITS clears the states and
# takes tag 1 (csrc/sa_onesweep.h kEpochBits, sa_build.hip next_epoch).
EPOCH_BITS = 14
EPOCH_LAST = (1 << EPOCH_BITS) - 1       # the largest tag; the pass after it wraps


def argsort_passes(bits: int) -> int:
    """Radix passes of one argsort (sa_sort_pairs_device) over `bits` key bits."""
    return (max(int(bits), 1) + 7) // 8


def advance_plan(epoch: int, target: int) -> list:
    """The `bits` of the argsort calls that take a context from tag `epoch`
    to tag `target` without wrapping: 8-pass calls (bits = 64), then 1-pass
    ones (bits = 8)."""
    if not 0 <= epoch <= target <= EPOCH_LAST:
        raise ValueError(f"cannot advance from {epoch} to {target}")
    d = target - epoch
    return [64] * (d // 8) + [8] * (d % 8)


def epoch_after(epoch: int, passes: int) -> int:
    """The tag of the last of `passes` further passes."""
    for _ in range(passes):
        epoch = 1 if epoch >= EPOCH_LAST else epoch + 1
    return epoch

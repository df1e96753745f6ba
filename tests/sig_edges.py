"""The crafted signature encodings of tests/golden/sig_edges.json (tools/gen_golden_sig_edges.py)
for the CPU and GPU tests of the signature-decoding routes.  Test infrastructure only."""
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ST_INFINITY = 100  # BGV_ST_INFINITY: the infinity encoding, skipped in the sums


def load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def corpus():
    """The entries, `sig` as bytes and `x` / `y` as integer pairs."""
    out = []
    for e in load("sig_edges.json")["entries"]:
        e = dict(e, sig=bytes.fromhex(e["sig"]))
        for k in ("x", "y"):
            if k in e:
                e[k] = tuple(int(v, 16) for v in e[k])
        out.append(e)
    return out


def golden_valid():
    """The valid golden signatures: (key index, root, signature)."""
    return [(c["key"], bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])) for c in load("signatures.json")["cases"]]


def owner(e, j, valid):
    """(key index, root) a set carrying entry e names: its own where the entry has one (a flipped or
    mixed golden signature), else those of the j-th valid golden signature."""
    if "key" in e:
        return e["key"], bytes.fromhex(e["msg"])
    return valid[j % len(valid)][:2]


def aggregate_lists():
    """The aggregation call of the fixture: [(name, [signature bytes], expect, aggregate or None)]."""
    d = load("sig_edges.json")
    sums = [bytes.fromhex(s) for s in d["sum_sigs"]]
    by_name = {e["name"]: bytes.fromhex(e["sig"]) for e in d["entries"]}

    def resolve(ref):
        if ref == "inf":
            return bytes([0xC0]) + bytes(95)
        if ref in by_name:
            return by_name[ref]
        s = sums[int(ref[1:])]
        return bytes([s[0] ^ 0x20]) + s[1:] if ref[0] == "f" else s

    return [(c["name"], [resolve(r) for r in c["sigs"]], c["expect"],
             bytes.fromhex(c["aggregate"]) if c["aggregate"] else None) for c in d["aggregates"]]


def place(n, edges, must):
    """Where the edge entries go among n sets: one at every slot of `must`, the rest spread evenly
    over the other slots, never two side by side beyond those, so that every 64-slot group keeps
    valid sets.  Returns {slot: entry}."""
    must = [s for s in must if s < n]
    assert len(edges) >= len(must) and 2 * len(edges) <= n + len(must)
    slots = dict(zip(must, edges))
    rest = edges[len(must):]
    free = [s for s in range(1, n - 1) if s not in slots and s - 1 not in slots and s + 1 not in slots]
    step = len(free) // max(1, len(rest))
    assert step >= 2 or not rest
    for k, e in enumerate(rest):
        slots[free[k * step]] = e
    assert len(slots) == len(edges)
    return slots


def decode_status(e):
    """What a decoding route reports for the entry: the BLST code, 100 for the infinity encoding."""
    return ST_INFINITY if e.get("infinity") else e["expect"]


def mismatches(entries, got, want=decode_status):
    """The names of the entries whose got value differs from want(entry); got runs parallel to
    entries and must cover them all."""
    got = list(got)
    assert len(got) == len(entries), (len(got), len(entries))
    return ["%s: got %r, want %r" % (e["name"], g, want(e)) for e, g in zip(entries, got) if g != want(e)]

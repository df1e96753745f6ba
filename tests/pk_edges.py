"""The crafted pubkey encodings of tests/golden/pk_edges.json (tools/gen_golden_pk_edges.py) for
the CPU and GPU tests of the pubkey-decoding routes.  Test infrastructure only."""
from tests.sig_edges import ST_INFINITY, load

PK_IS_INFINITY = 6  # what a cache put and the key validation report for an infinity encoding
INF96 = bytes([0x40]) + bytes(95)


def fixture():
    return load("pk_edges.json")


def corpus():
    """The entries, wire forms as bytes and `x` / `y` as integers."""
    out = []
    for e in fixture()["entries"]:
        e = dict(e)
        for k in ("pk48", "pk96", "root", "sig", "agg_sig"):
            if k in e:
                e[k] = bytes.fromhex(e[k])
        for k in ("x", "y"):
            if k in e:
                e[k] = int(e[k], 16)
        out.append(e)
    return out


def with_form(entries, form):
    """The entries that have the wire form (48 or 96)."""
    return [e for e in entries if "pk%d" % form in e]


def decode_status(e, form):
    """What a decoding of the entry's wire form reports: the BLST code, 100 for an infinity encoding."""
    return ST_INFINITY if e.get("infinity%d" % form) else e["expect%d" % form]


def put_status(e, form):
    """The code bgv_pubkeys_put has for the entry: an infinity encoding is no usable key."""
    return PK_IS_INFINITY if e.get("infinity%d" % form) else e["expect%d" % form]


def point(e):
    return (e["x"], e["y"]) if "x" in e else None


def job_code(e):
    """The code of a one-set job whose only key is the entry's 96-byte record."""
    if e["expect96"]:
        return -e["expect96"]
    return 0 if e.get("infinity96") else e["verdict"]


def keys():
    k = load("keys.json")
    return k, [bytes.fromhex(h) for h in k["pk_uncompressed"]]


def record(ref, by_name, pk96, o):
    """The 96 bytes a record reference of the fixture's sets stands for (o: the oracle, for the
    encodings only)."""
    if ref == "inf":
        return INF96
    if ref == "cinf":
        return bytes([0xC0]) + bytes(95)
    if ref in by_name:
        return by_name[ref]["pk96"]
    j = int(ref[1:])
    if ref[0] == "k":
        return pk96[j]
    pt = o.g1_deserialize(pk96[j])
    if ref[0] == "n":
        return o.g1_serialize(o.g1_neg(pt))
    assert ref[0] == "c"
    return o.g1_compress(pt) + bytes(48)


def record_sets(o):
    """The fixture's multi-record sets and the partner of the two-set jobs, references resolved:
    ([{name, records, root, sig, expect, pair_expect}], partner)."""
    fx = fixture()
    _, pk96 = keys()
    by_name = {e["name"]: e for e in corpus()}

    def resolve(s):
        return dict(s, records=[record(r, by_name, pk96, o) for r in s["records"]], refs=s["records"],
                    root=bytes.fromhex(s["root"]), sig=bytes.fromhex(s["sig"]))

    return [resolve(s) for s in fx["sets"]], resolve(fx["pair_partner"])

"""CPU checks of the committee-bitfield sets (include/blsgpu.h bgv_verify_bits): the per-lane
selection and the mode decision of bgv_pk_bits.h with the host build of the G1 arithmetic, and
the host layout of calls that hold committee sets (bgv_host_layout.h), through
tests/native/committeesim.cpp.  Expected aggregates come from the oracle
(tests/golden/committee_bits.json, tools/gen_golden_committee.py)."""
import pytest

from tests import committeesim as cs

MODES = {0: "direct", 1: "complement", 2: "derived"}


@pytest.fixture(scope="module")
def aggregates():
    """Every fixture case on teams of 16 and 64 lanes in both forced modes and the derived one:
    {(case name, T, mode): (aggregate hex, complement taken)}; one simulator run."""
    fx = cs.fixture()
    lines = ["keys %d" % len(fx["keys"])] + fx["keys"]
    order = []
    for c in fx["cases"]:
        members = fx["committees"][c["committee"]]
        for T in (16, 64):
            for mode in MODES:
                lines.append("case %d %d %d %s %s" % (T, mode, c["n"], c["bits"], " ".join(map(str, members))))
                order.append((c["name"], T, mode))
    out = cs.run("agg", "\n".join(lines) + "\n")
    assert len(out) == len(order)
    return {key: (line.split()[0], int(line.split()[1])) for key, line in zip(order, out)}


def test_fixture_shape():
    fx = cs.fixture()
    assert len(fx["keys"]) == 521
    sizes = {c["n"] for c in fx["cases"] if c["committee"].startswith("n")}
    assert sizes == {1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 257, 512, 513}
    for c in fx["cases"]:
        assert c["k"] == sum(bin(b).count("1") for b in bytes.fromhex(c["bits"])) >= 1
        assert len(fx["committees"][c["committee"]]) == c["n"]
    # infinity aggregates are among the cases
    assert any(c["agg"] == "40" + "00" * 95 for c in fx["cases"])


@pytest.mark.parametrize("T", [16, 64])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_selection_matches_oracle(aggregates, T, mode):
    """Lane l takes the selected members of rank l, l + T, ...; the lanes' sums combined (and
    subtracted from the total in complement mode) are the oracle's aggregate, byte for byte."""
    for c in cs.fixture()["cases"]:
        got, comp = aggregates[(c["name"], T, mode)]
        assert got == c["agg"], (c["name"], T, MODES[mode])
        if mode == 2:  # the rule: complement iff n - k + 1 < k
            assert comp == int(c["n"] - c["k"] + 1 < c["k"]), c["name"]


COMMITTEES = {7: (1007, 128, 0), 8: (1008, 1, 0), 9: (1009, 600, 0), 10: (1010, 16, 1)}
EVEN128 = list(range(0, 128, 2))


def _scenario():
    """Two calls of one-set jobs; per set ("idx", indices) or ("com", id, n_bits, positions)."""
    call1 = [
        ("idx", [3, 4, 5]),
        ("com", 7, 128, EVEN128),                # k = 64: direct
        ("com", 7, 128, EVEN128 + [1]),          # k = 65: complement
        ("com", 8, 1, [0]),                      # n = 1, k = 1: direct
        ("com", 9, 600, list(range(0, 600, 2))),  # k = 300: direct, 300 terms: a wave
        ("com", 9, 600, list(range(10, 600))),   # k = 590: complement, 10 terms: a team
        ("com", 99, 128, EVEN128),               # unknown id
        ("com", 7, 127, list(range(0, 127, 2))),  # n_bits is not the committee's length
        ("com", 8, 1, "03"),                     # a set bit past n_bits in the last byte
        ("com", 7, 128, []),                     # no bit set
        ("com", 10, 16, [0, 1]),                 # the committee holds a marked key
    ]
    call2 = [("idx", [9, 10]), ("com", 7, 128, EVEN128 + [1])]
    return [call1, call2]


def _bits(s):
    return bytes.fromhex(s[3]) if isinstance(s[3], str) else cs.pack(s[3], s[2])


def _layout_text():
    lines = ["committee %d %d %d %d" % (i, h, n, bad) for i, (h, n, bad) in COMMITTEES.items()]
    for call in _scenario():
        lines.append("call 1")
        for s in call:
            if s[0] == "idx":
                lines.append("set idx %d %s" % (len(s[1]), " ".join(map(str, s[1]))))
            else:
                lines.append("set com %d %d %s" % (s[1], s[2], _bits(s).hex() or "-"))
        lines.append("end")
    return "\n".join(lines) + "\n"


def _parse(lines):
    calls, merged = [], {"mslot": [], "midx": [], "mcom": []}
    for ln in lines:
        w = ln.split()
        if w[0] == "code":
            if int(w[1]) == 0:
                calls.append({"code": [], "slot": [], "idx": None, "team": None, "wave": None})
            calls[-1]["code"].append(int(w[2]))
        elif w[0] == "slot":
            calls[-1]["slot"].append(tuple(int(v) for v in w[1:]))
        elif w[0] in ("idx", "team", "wave"):
            calls[-1][w[0]] = [int(v) for v in w[1:]]
        elif w[0] == "mslot":
            merged["mslot"].append(tuple(int(v) for v in w[1:]))
        else:
            merged[w[0]] = [int(v) for v in w[1:]]
    return calls, merged


@pytest.fixture(scope="module")
def layout():
    return _parse(cs.run("layout", _layout_text()))


def test_layout_argument_errors_leave_no_slot(layout):
    calls, _ = layout
    assert calls[0]["code"] == [2, 2, 2, 2, 2, 2, -cs.E_BAD_INDEX, -cs.E_ARG, -cs.E_ARG, -cs.E_EMPTY_AGGREGATE,
                                -cs.E_BAD_INDEX]
    assert calls[1]["code"] == [2, 2]
    # only the sets that passed have a slot
    assert [s[1] for s in calls[0]["slot"]] == [0, 1, 2, 3, 4, 5]
    assert [s[1] for s in calls[1]["slot"]] == [0, 1]


def test_layout_handle_words_and_mode(layout):
    calls, _ = layout
    for call, sets in zip(calls, _scenario()):
        idx = call["idx"]
        for slot, si, flags, n_pk, pk_off, group in call["slot"]:
            s = sets[si]
            if s[0] == "idx":
                assert flags == cs.PK_CACHED and n_pk == len(s[1]) and idx[pk_off:pk_off + n_pk] == s[1]
                continue
            handle, n, _ = COMMITTEES[s[1]]
            bits = _bits(s)
            k = sum(bin(b).count("1") for b in bits)
            comp = n - k + 1 < k
            assert flags == cs.PK_COMMITTEE | (cs.PK_COMPLEMENT if comp else 0), (si, flags)
            assert n_pk == k
            assert idx[pk_off] == handle  # the committee's device handle, then the bit words
            words = cs.words_of(bits, n)
            assert idx[pk_off + 1:pk_off + 1 + len(words)] == words
            terms = n - k if comp else k
            assert (slot in call["team"]) == (terms <= cs.PK_TEAM_MAX)
            assert (slot in call["wave"]) == (terms > cs.PK_TEAM_MAX)
    flags = {si: f for _, si, f, *_ in calls[0]["slot"]}
    assert flags[1] == cs.PK_COMMITTEE                      # n = 128, k = 64
    assert flags[2] == cs.PK_COMMITTEE | cs.PK_COMPLEMENT   # n = 128, k = 65
    assert flags[3] == cs.PK_COMMITTEE                      # n = 1, k = 1
    assert len(calls[0]["wave"]) == 1 and len(calls[0]["team"]) == 4
    # the index array holds nothing but the runs
    assert len(calls[0]["idx"]) == 3 + (1 + 4) * 2 + (1 + 1) + (1 + 19) * 2


def test_layout_merged_call_rebases(layout):
    calls, merged = layout
    n1 = len(calls[0]["idx"])
    base = 64 * len(calls[0]["slot"])  # every one-set job owns a group: one wave of slots each
    want = [(s, f, k, off, g) for s, _, f, k, off, g in calls[0]["slot"]]
    want += [(s + base, f, k, off + n1, g + len(calls[0]["slot"])) for s, _, f, k, off, g in calls[1]["slot"]]
    assert merged["mslot"] == want
    assert merged["midx"] == calls[0]["idx"] + calls[1]["idx"]
    # the merged committee list: the teams of every call, then the waves
    assert merged["mcom"] == calls[0]["team"] + [s + base for s in calls[1]["team"]] + calls[0]["wave"]
    # the second call's committee slot still finds its handle and words
    s, f, k, off, g = merged["mslot"][-1]
    assert merged["midx"][off] == 1007
    assert merged["midx"][off + 1:off + 5] == cs.words_of(cs.pack(EVEN128 + [1], 128), 128)


def test_sanitizer_build_agrees():
    """The layout checks' driver under AddressSanitizer and UBSan (a stand-alone CPU program
    without the G1 arithmetic): same output as the plain build, no report."""
    text = _layout_text()
    assert cs.run("layout", text, "san") == cs.run("layout", text, "O2")


def test_python_committee_set_form():
    """ISignatureSet's committee form -> SetSpec -> the bgv_pkbits array beside the sets."""
    from lodestar_amd import native, verifier as v
    s = v.ISignatureSet(v.SignatureSetType.committee, bytes(32), bytes(96), committee=3, bits=bytes([0x1F, 0x01]),
                        n_bits=9)
    plain = v.ISignatureSet(v.SignatureSetType.aggregate, bytes(32), bytes(96), pubkeys=[4, 5])
    assert v.get_aggregated_pubkeys_count([s, plain]) == 6 + 2
    packed = native.PackedCall([([v.to_set_spec(s), v.to_set_spec(plain)], False)])
    assert packed.pkbits[0].committee == 3 and packed.pkbits[0].n_bits == 9
    assert packed.pkbits[1].committee == native.NO_COMMITTEE
    assert native.PackedCall([([v.to_set_spec(plain)], False)]).pkbits is None  # bgv_verify as before
    with pytest.raises(ValueError):
        native.SetSpec(bytes(32), bytes(96), committee=3, bits=bytes(1), n_bits=9)  # too few bytes
    with pytest.raises(ValueError):
        native.SetSpec(bytes(32), bytes(96), committee=3, bits=bytes(2), n_bits=9, pk_indices=[1])

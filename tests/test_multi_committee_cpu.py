"""CPU checks of the span sets (include/blsgpu.h bgv_verify_spans: one bitfield over several
device-resident committees): the host's cut of the bitfield and the per-lane walk of
bgv_pk_bits.h with the host build of the G1 arithmetic, and the host checks and layout of calls
that hold span sets (bgv_host_layout.h), through tests/native/multicomsim.cpp.  Expected
aggregates come from the oracle (tests/golden/multi_committee.json,
tools/gen_golden_multi_committee.py)."""
import pytest

from tests import committeesim as cs
from tests import multicomsim as ms


def test_fixture_shape():
    fx = ms.fixture()
    by = {c["name"]: c for c in fx["cases"]}
    assert by["n17_n33"]["committees"] == ["n17", "n33"]
    assert by["n1_n31_n1_n65"]["committees"] == ["n1", "n31", "n1", "n65"]
    assert len(by["sixty_four"]["committees"]) == ms.MAX_SET_COMMITTEES
    assert {by[n]["terms"] for n in ("m16", "m17", "m48", "m49", "m256", "m257")} == {16, 17, 48, 49, 256, 257}
    for c in fx["cases"]:
        bits = bytes.fromhex(c["bits"])
        assert c["n_bits"] == sum(len(fx["committees"][n]) for n in c["committees"])
        assert len(bits) == (c["n_bits"] + 7) // 8
        assert c["k"] == sum(bin(b).count("1") for b in bits) == len(ms.expand(c)) >= 1
    # only the last word of the bitfield holds bits
    lw = by["last_word"]
    assert cs.words_of(bytes.fromhex(lw["bits"]), lw["n_bits"])[:-1] == [0] * ((lw["n_bits"] + 31) // 32 - 1)
    assert sum(c["agg"] == "40" + "00" * 95 for c in fx["cases"]) >= 2  # infinity results


@pytest.fixture(scope="module")
def aggregates():
    """Every fixture case on teams of 16 and 64 lanes: {(name, T): (aggregate hex, M)}; one run."""
    fx = ms.fixture()
    handle = {name: 100 + i for i, name in enumerate(sorted(fx["committees"]))}
    lines = ["keys %d" % len(fx["keys"])] + fx["keys"]
    for name, members in fx["committees"].items():
        lines.append("committee %d %d %s" % (handle[name], len(members), " ".join(map(str, members))))
    order = []
    for c in fx["cases"]:
        for T in (16, 64):
            lines.append("case %d %d %s %d %s" % (T, c["n_bits"], c["bits"], len(c["committees"]),
                                                 " ".join(str(handle[n]) for n in c["committees"])))
            order.append((c["name"], T))
    out = ms.run("agg", "\n".join(lines) + "\n")
    assert len(out) == len(order)
    return {key: (line.split()[0], int(line.split()[1])) for key, line in zip(order, out)}


@pytest.mark.parametrize("T", [16, 64])
def test_walk_matches_oracle(aggregates, T):
    """Lane l takes the terms of rank l, l + T, ... of the whole span (the simulator checks each
    lane's count, ceil((M - l) / T)); the lanes' sums combined are the oracle's aggregate of the
    expanded index list, byte for byte, and M is the fixture's term count."""
    for c in ms.fixture()["cases"]:
        got, m = aggregates[(c["name"], T)]
        assert got == c["agg"], (c["name"], T)
        assert m == c["terms"], c["name"]


# id -> (handle, members, holds a marked key)
COMMITTEES = {7: (1007, 128, 0), 8: (1008, 1, 0), 9: (1009, 600, 0), 10: (1010, 16, 1), 11: (1011, 17, 0),
              12: (1012, 33, 0), 13: (1013, 65536, 0)}
EVEN128 = list(range(0, 128, 2))


def _span(ids, per):
    """("span", ids, n_bits, positions over the concatenation); per: positions inside each committee"""
    pos, off = [], 0
    for i, sel in zip(ids, per):
        pos += [off + p for p in sel]
        off += COMMITTEES[i][1]
    return ("span", list(ids), off, pos)


GOOD = [
    _span([11, 12], [[0, 5, 16], list(range(3, 33))]),             # 17 then 33: direct 3, complement 3 + total
    _span([8, 7, 8], [[0], EVEN128 + [1], [0]]),                   # a repeated one-member committee
    _span([9, 7, 11], [list(range(0, 600, 2)), [], list(range(17))]),  # 300 + 0 + total: a wave
    ("span", [7], 128, EVEN128 + [1]),                             # one committee: the committee slot itself
]


def _errors():
    one = COMMITTEES[8][1]
    return [
        (("span", [7, 99], 160, EVEN128), -cs.E_BAD_INDEX),                        # 1: an unknown id
        (("span", [8] * 70 + [99], 5, [0]), -cs.E_BAD_INDEX),                      # 1 before 2: unknown past 64
        (("span", [7, 99], 3, "ff"), -cs.E_BAD_INDEX),                             # 1 before 2 and 3
        (("span", [8] * 65, 65 * one, [0]), -cs.E_ARG),                            # 2: more than 64 committees
        (("span", [13, 13, 13], 3 * 65536, [0]), -cs.E_ARG),                       # 2: more than 131,072 bits
        (("span", [11, 12], 49, [0]), -cs.E_ARG),                                  # 2: n_bits is not 17 + 33
        (("span", [11, 12], 50, "000000000000fc"), -cs.E_ARG),                     # 3: set bits at and past bit 50
        (("span", [11, 10], 33, "0000000002"), -cs.E_ARG),                         # 3 before 4 and 5
        (_span([11, 12], [[], []]), -cs.E_EMPTY_AGGREGATE),                        # 4: no bit set
        (_span([11, 10], [[], []]), -cs.E_EMPTY_AGGREGATE),                        # 4 before 5
        (_span([11, 10], [[1], []]), -cs.E_BAD_INDEX),                             # 5: a listed committee is marked
    ]


def _bits(s):
    return bytes.fromhex(s[3]) if isinstance(s[3], str) else cs.pack(s[3], s[2])


def _text(calls):
    lines = ["committee %d %d %d %d" % (i, h, n, bad) for i, (h, n, bad) in COMMITTEES.items()]
    for call in calls:
        lines.append("call 1")
        for s in call:
            if s[0] == "idx":
                lines.append("set idx %d %s" % (len(s[1]), " ".join(map(str, s[1]))))
            elif s[0] == "com":
                lines.append("set com %d %d %s" % (s[1], s[2], _bits(s).hex() or "-"))
            else:
                lines.append("set span %d %s %d %s" % (s[2], _bits(s).hex() or "-", len(s[1]), " ".join(map(str, s[1]))))
        lines.append("end")
    return "\n".join(lines) + "\n"


def _parse(lines):
    calls, merged = [], {"mslot": []}
    for ln in lines:
        w = ln.split()
        if w[0] == "code":
            if int(w[1]) == 0:
                calls.append({"code": [], "slot": []})
            calls[-1]["code"].append(int(w[2]))
        elif w[0] == "slot":
            calls[-1]["slot"].append(tuple(int(v) for v in w[1:]))
        elif w[0] == "mslot":
            merged["mslot"].append(tuple(int(v) for v in w[1:]))
        elif w[0].startswith("m"):
            merged[w[0]] = [int(v) for v in w[1:]]
        else:
            calls[-1][w[0]] = [int(v) for v in w[1:]]
    return calls, merged


def _calls():
    call1 = [("idx", [3, 4, 5])] + GOOD + [s for s, _ in _errors()]
    call2 = [("idx", [9, 10]), GOOD[0], ("com", 7, 128, EVEN128)]
    call3 = [("com", 7, 128, EVEN128 + [1])]  # no span in the call: committee_set_check, as bgv_verify_bits
    return [call1, call2, call3]


@pytest.fixture(scope="module")
def layout():
    return _parse(ms.run("layout", _text(_calls())))


def _want_run(s):
    """The span's run as bgv_pk_bits.h documents it, and M, from the set itself."""
    bits, off, comp_handles, recs, m = _bits(s), 0, [], [], 0
    bit = lambda p: (bits[p >> 3] >> (p & 7)) & 1  # noqa: E731
    for i in s[1]:
        handle, n, _ = COMMITTEES[i]
        sel = [bit(off + p) for p in range(n)]
        k = sum(sel)
        comp = n - k + 1 < k
        if comp:
            comp_handles.append(handle)
            sel = [1 - b for b in sel]
        m += sum(sel) + comp
        for w in range((n + 31) // 32):
            v = sum(b << q for q, b in enumerate(sel[32 * w:32 * w + 32]))
            if v:
                recs += [v, handle | w << 15 | comp << 31]
        off += n
    return [len(recs) // 2, len(comp_handles), m] + comp_handles + recs, m


def test_layout_codes_in_order_and_no_slot_on_error(layout):
    calls, _ = layout
    want = [2] * (1 + len(GOOD)) + [code for _, code in _errors()]
    assert calls[0]["code"] == want
    # only the sets that passed have a slot
    assert [s[1] for s in calls[0]["slot"]] == list(range(1 + len(GOOD)))
    assert calls[1]["code"] == [2, 2, 2] and calls[2]["code"] == [2]


def test_layout_run_flags_and_lists(layout):
    calls, _ = layout
    sets = _calls()[0]
    idx = calls[0]["idx"]
    used = 0
    for slot, si, flags, n_pk, pk_off, group in calls[0]["slot"]:
        s = sets[si]
        if s[0] == "idx":
            assert flags == cs.PK_CACHED and idx[pk_off:pk_off + n_pk] == s[1]
            used += n_pk
            continue
        assert n_pk == sum(bin(b).count("1") for b in _bits(s))  # n_pk stays the number of set bits
        if len(s[1]) == 1:
            continue  # test_one_committee_span_is_the_committee_slot
        run, m = _want_run(s)
        assert flags == cs.PK_COMMITTEE | ms.PK_SPAN, (si, flags)
        assert idx[pk_off:pk_off + len(run)] == run, si
        assert (slot in calls[0]["steam"]) == (m <= cs.PK_TEAM_MAX)
        assert (slot in calls[0]["swave"]) == (m > cs.PK_TEAM_MAX)
        assert slot not in calls[0]["team"] + calls[0]["wave"]
        used += len(run)
    assert len(calls[0]["swave"]) == 1 and len(calls[0]["steam"]) == 2
    assert used + 1 + 4 == len(idx)  # nothing but the runs (and the one-committee span's handle and words)


def test_one_committee_span_is_the_committee_slot(layout):
    """n_committees == 1 lays out the very slot bgv_verify_bits does: flags, n_pk, handle, words, side."""
    calls, _ = layout
    via_span = next(s for s in calls[0]["slot"] if s[1] == len(GOOD))  # ("span", [7], ...)
    via_bits = calls[2]["slot"][0]
    assert via_span[2:4] == via_bits[2:4] == (cs.PK_COMMITTEE | cs.PK_COMPLEMENT, 65)
    a, b = via_span[4], via_bits[4]
    assert calls[0]["idx"][a:a + 5] == calls[2]["idx"][b:b + 5] == [1007] + cs.words_of(cs.pack(EVEN128 + [1], 128), 128)
    assert via_span[0] in calls[0]["team"] and calls[2]["team"] == [via_bits[0]]
    # and a "com" set beside a span in one spans array (call 2) is the same slot again
    com = calls[1]["slot"][2]
    assert com[2:4] == (cs.PK_COMMITTEE, 64) and calls[1]["idx"][com[4]] == 1007


def test_layout_merged_call_rebases(layout):
    calls, merged = layout
    want, sb, ib, gb = [], 0, 0, 0
    for call in calls:
        want += [(s + sb, f, k, off + ib, g + gb) for s, _, f, k, off, g in call["slot"]]
        sb += 64 * len(call["slot"])  # every one-set job owns a group: one wave of slots each
        ib += len(call["idx"])
        gb += len(call["slot"])
    assert merged["mslot"] == want
    assert merged["midx"] == calls[0]["idx"] + calls[1]["idx"] + calls[2]["idx"]
    b1, b2 = 64 * len(calls[0]["slot"]), 64 * (len(calls[0]["slot"]) + len(calls[1]["slot"]))
    assert merged["mlist"] == (calls[0]["team"] + [s + b1 for s in calls[1]["team"]] + [s + b2 for s in calls[2]["team"]]
                               + calls[0]["wave"]
                               + calls[0]["steam"] + [s + b1 for s in calls[1]["steam"]] + calls[0]["swave"])
    # the second call's span slot still finds its run: the records hold handles, no offsets
    s, f, k, off, g = merged["mslot"][len(calls[0]["slot"]) + 1]
    run, _ = _want_run(GOOD[0])
    assert f == cs.PK_COMMITTEE | ms.PK_SPAN and merged["midx"][off:off + len(run)] == run


def test_sanitizer_build_agrees():
    """The layout driver under AddressSanitizer and UBSan (a stand-alone CPU program without the
    G1 arithmetic): same output as the plain build, no report."""
    text = _text(_calls())
    assert ms.run("layout", text, "san") == ms.run("layout", text, "O2")


def test_python_span_set_form():
    """ISignatureSet's committees form -> SetSpec -> the bgv_pkspan array beside the sets."""
    from lodestar_amd import native, verifier as v
    s = v.ISignatureSet(v.SignatureSetType.committees, bytes(32), bytes(96), committees=[3, 9],
                        bits=bytes([0x1F, 0x01]), n_bits=9)
    one = v.ISignatureSet(v.SignatureSetType.committee, bytes(32), bytes(96), committee=4, bits=bytes([3]), n_bits=2)
    plain = v.ISignatureSet(v.SignatureSetType.aggregate, bytes(32), bytes(96), pubkeys=[4, 5])
    assert v.get_aggregated_pubkeys_count([s, one, plain]) == 6 + 2 + 2
    packed = native.PackedCall([([v.to_set_spec(s), v.to_set_spec(one), v.to_set_spec(plain)], False)])
    assert packed.pkbits is None
    assert [packed.spans[i].n_committees for i in range(3)] == [2, 1, 0]
    assert packed.spans[0].n_bits == 9 and packed.sets[0].n_pk == 6
    # a list of one id is the committee set: no spans array, bgv_verify_bits as before
    single = native.SetSpec(bytes(32), bytes(96), committees=[4], bits=bytes([3]), n_bits=2)
    assert single.committee == 4 and single.committees is None
    p1 = native.PackedCall([([single], False)])
    assert p1.spans is None and p1.pkbits[0].committee == 4
    with pytest.raises(ValueError):
        native.SetSpec(bytes(32), bytes(96), committees=[], bits=bytes(1), n_bits=1)
    with pytest.raises(ValueError):
        native.SetSpec(bytes(32), bytes(96), committees=[1, 2], committee=1, bits=bytes(1), n_bits=1)
    with pytest.raises(ValueError):
        native.SetSpec(bytes(32), bytes(96), committees=[1, 2], bits=bytes(1), n_bits=9)  # too few bytes
    for name in ("bgv_verify_spans", "bgv_verify_spans_async", "bgv_aggregate_span"):
        assert name in native.EXPORTED_SYMBOLS

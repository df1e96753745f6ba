"""Builds and runs tests/native/sigpoolbitssim.cpp, the CPU driver of the host plan of pool entries
with participation bits (bgv_sigpool_bits_plan.h), and holds the Python model its checks, plan,
commit and bit concatenation are compared with.  The model is written from the contract in
include/blsgpu.h, with fields as Python sets of positions.  Test infrastructure only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sigpoolbitssim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "bgv_sigpool_bits_plan.h"), os.path.join(CSRC, "bgv_sigpool_plan.h"),
        os.path.join(CSRC, "bgv_sigagg_plan.h"), os.path.join(os.path.dirname(HERE), "include", "blsgpu.h")]
BUILDS = {
    "O2": ["-O2"],
    "san": ["-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
NO_AGG = 0xFFFFFFFF
E_BAD_INDEX, E_ARG = 22, 23
FORM_NONE, FORM_WAVE, FORM_BULK = 0, 1, 2
NOT_ADDED, ADDED, KNOWN, OVERLAP = 0, 1, 2, 3


def build(kind="O2"):
    out = os.path.join(HERE, "native", "sigpoolbitssim_" + kind)
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in DEPS):
        return out
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-o", out + ".tmp", SRC] + BUILDS[kind])
    os.replace(out + ".tmp", out)
    return out


def consts(kind="O2"):
    """(NO_AGG, SIGAGG_WAVE_MAX, MAX_SIGPOOL, SIGPOOL_MAX_BITS, SIGPOOL_BITS_BYTES, MAX_SUM_ENTRIES,
    NOT_ADDED, ADDED, KNOWN, OVERLAP) as the headers define them."""
    return tuple(int(v) for v in subprocess.check_output([build(kind), "consts"], text=True).split())


def to_hex(positions, n_bits):
    """SSZ bit order: position k is bit k % 8 of byte k // 8.  Positions at or past n_bits land in
    the last byte when they fit in it (the stray-bit cases)."""
    b = bytearray((n_bits + 7) // 8)
    for k in positions:
        b[k // 8] |= 1 << (k % 8)
    return b.hex() or "-"


def from_hex(text, n_bits):
    if text == "-":
        return frozenset()
    b = bytes.fromhex(text)
    return frozenset(k for k in range(len(b) * 8) if b[k // 8] >> (k % 8) & 1)


class Member:
    """bits_of_set[i]: n_bits, and either a single position (bits == NULL) or a field (positions;
    one at or past n_bits that still fits the last byte is a stray bit)."""

    def __init__(self, n_bits, bit=None, field=None):
        self.n_bits, self.bit, self.field = n_bits, bit, None if field is None else frozenset(field)

    def line(self):
        if self.field is None:
            return "%d %d -" % (self.n_bits, self.bit)
        return "%d 0 %s" % (self.n_bits, to_hex(self.field, self.n_bits))


class Entry:
    """A registry entry: generation, count, n_bits (0: plain) and the positions set."""

    def __init__(self, gen=1, count=0, n_bits=0, bits=(), live=1):
        self.gen, self.count, self.n_bits, self.bits, self.live = gen, count, n_bits, frozenset(bits), live

    def line(self, i, with_live):
        head = "%d %d" % (i, self.live) if with_live else "%d" % i
        return "%s %d %d %d %s" % (head, self.gen, self.count, self.n_bits, to_hex(self.bits, self.n_bits))


def run(cases, kind="O2"):
    """cases: [(jobs, tags, members, entries, changed, flags, wave_max)] with jobs = [(first_set,
    n_sets, code)], members = None (bits_of_set NULL) or one Member per set, entries = {id: Entry}
    at submit, changed = {id: Entry} before the step, flags = {id: code} the device reports.
    Returns per case -code, or (form, ids, first, count, member, outcome, registry) with registry
    = {id: (count, n_bits, positions)} of the live entries after the commit."""
    text = ["%d" % len(cases)]
    for jobs, tags, members, entries, changed, flags, wave_max in cases:
        text.append("%d %d %d %d %d %d %d" % (len(jobs), len(tags), len(entries), len(changed), len(flags), wave_max,
                                              members is not None))
        text += ["%d %d %d" % j for j in jobs]
        text.append(" ".join("%d" % t for t in tags))
        if members is not None:
            text += [m.line() for m in members]
        text += [e.line(i, False) for i, e in entries.items()]
        text += [e.line(i, True) for i, e in changed.items()]
        text += ["%d %d" % kv for kv in flags.items()]
    p = subprocess.run([build(kind)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, "sigpoolbitssim (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        f = line.split("|")
        head = [int(v) for v in f[0].split()]
        if head[0] != 0:
            out.append(head[0])
            continue
        ids, first, count, member, outcome = ([int(v) for v in g.split()] for g in f[1:6])
        assert len(member) == head[2]
        reg = {}
        for item in f[6].split():
            i, cnt, nb, hx = item.split(":")
            reg[int(i)] = (int(cnt), int(nb), from_hex(hx, int(nb)))
        out.append((head[1], ids, first, count, member, outcome, reg))
    assert len(out) == len(cases)
    return out


def model(jobs, tags, members, entries, changed, flags, wave_max, max_pool=16384):
    """Submit: the tag checks of bgv_verify_accumulate; then for every tagged set whose entry has
    bits -E_ARG when there is no bits_of_set, n_bits differs, the single position is not below
    n_bits, a field has a position at or past n_bits or is empty.  Step: per entry, members in set
    order against the entry's positions as the step finds them: disjoint -> added, within ->
    known, else overlap.  Commit: a flagged entry keeps everything and all its sets report 0."""
    if any(t != NO_AGG and t >= max_pool for t in tags):
        return -E_ARG
    if any(t != NO_AGG and t not in entries for t in tags):
        return -E_BAD_INDEX
    for i, t in enumerate(tags):
        if t == NO_AGG or entries[t].n_bits == 0:
            continue
        n = entries[t].n_bits
        if members is None or members[i].n_bits != n:
            return -E_ARG
        m = members[i]
        if m.field is None:
            if m.bit >= n:
                return -E_ARG
        elif not m.field or max(m.field) >= n:
            return -E_ARG
    gens = [0 if t == NO_AGG else entries[t].gen for t in tags]
    now = dict(entries)
    now.update(changed)
    accepted = set()
    for first, n, code in jobs:
        if code == 1:
            accepted.update(range(first, first + n))
    outcome = [NOT_ADDED] * len(tags)
    work, by_id = {}, {}
    for i in sorted(accepted):
        t = tags[i]
        if t == NO_AGG or not now[t].live or now[t].gen != gens[i]:
            continue
        if now[t].n_bits == 0:
            outcome[i] = ADDED
        else:
            b = work.setdefault(t, set(now[t].bits))
            m = {members[i].bit} if members[i].field is None else set(members[i].field)
            if not (m & b):
                outcome[i] = ADDED
                b |= m
            else:
                outcome[i] = KNOWN if m <= b else OVERLAP
        if outcome[i] == ADDED:
            by_id.setdefault(t, []).append(i)
    ids = sorted(by_id)
    member = [i for e in ids for i in by_id[e]]
    first, at = [], 0
    for e in ids:
        first.append(at)
        at += len(by_id[e])
    form = FORM_NONE if not member else FORM_WAVE if len(member) <= wave_max else FORM_BULK
    reg = {i: (e.count, e.n_bits, e.bits) for i, e in now.items() if e.live}
    for e in ids:
        if flags.get(e, 0) != 0:
            for i, t in enumerate(tags):
                if t == e:
                    outcome[i] = NOT_ADDED
            continue
        cnt, nb, bits = reg[e]
        reg[e] = (cnt + len(by_id[e]), nb, frozenset(work[e]) if nb else bits)
    return form, ids, first, [len(by_id[e]) for e in ids], member, outcome, reg


def run_concat(lists, kind="O2"):
    """lists: [[(n_bits, positions)]]; returns per list (total_bits, bytes) of the driver's
    concatenation."""
    text = ["%d" % len(lists)]
    for items in lists:
        text.append("%d" % len(items))
        text += ["%d %s" % (n, to_hex(pos, n)) for n, pos in items]
    p = subprocess.run([build(kind), "concat"], input="\n".join(text) + "\n", capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, "sigpoolbitssim concat (%s) exit %d: %s" % (kind, p.returncode, p.stderr[-2000:])
    out = []
    for line in p.stdout.splitlines():
        total, hx = line.split()
        out.append((int(total), b"" if hx == "-" else bytes.fromhex(hx)))
    assert len(out) == len(lists)
    return out


def model_concat(items):
    """Bit by bit: entry c owns positions [off_c, off_c + n_c)."""
    total = sum(n for n, _ in items)
    out = bytearray((total + 7) // 8)
    off = 0
    for n, pos in items:
        for k in range(n):
            if k in pos:
                out[(off + k) // 8] |= 1 << ((off + k) % 8)
        off += n
    return total, bytes(out)

"""The one-shot calls' device-memory owner on a CPU: bgv_devscope.h's DevScope over a recording
policy, run by tests/native/devscopesim.cpp through calls scripted like the library's.  Checked:
every allocation is freed exactly once on every path, the stream is drained exactly once and
before the first free, the success path issues its explicit synchronize only, release() keeps a
buffer out of the frees, and an idle scope touches nothing.  Every case also runs in the
simulator's address/undefined sanitizer build, whose policy memory is real heap memory."""
import pytest

from tests import devscopesim as S

KINDS = ["O2", "san"]


def frees(log):
    return [e for e in log if e[0] == "f"]


def drains_before_frees(log):
    """exactly one synchronize, and no free before it"""
    return log.count("s") == 1 and all(log.index("s") < i for i, e in enumerate(log) if e[0] == "f")


@pytest.mark.parametrize("kind", KINDS)
def test_allocation_failure_frees_what_succeeded(kind):
    got = S.run(["call %d -1" % k for k in range(S.NALLOC)], kind)
    for k, (rc, log) in enumerate(got):
        assert rc == -S.BGV_E_DEVICE, k
        assert [e for e in log if e[0] in "ax"] == ["a%d" % i for i in range(k)] + ["x%d" % k], (k, log)
        assert frees(log) == ["f%d" % i for i in range(k)], (k, log)  # each once, in allocation order
        assert not [e for e in log if e[0] in "oy"], (k, log)  # nothing was enqueued
        if k:
            assert drains_before_frees(log), (k, log)
        else:
            assert log == ["x0"]


@pytest.mark.parametrize("kind", KINDS)
def test_failure_after_j_operations_drains_once_before_the_frees(kind):
    got = S.run(["call -1 %d" % j for j in range(S.NOPS + 1)], kind)
    for j, (rc, log) in enumerate(got):
        assert rc == -S.BGV_E_DEVICE, j
        assert [e for e in log if e[0] == "o"] == ["o%d" % i for i in range(min(j, S.NOPS))], (j, log)
        assert drains_before_frees(log), (j, log)
        assert frees(log) == ["f%d" % i for i in range(S.NALLOC)], (j, log)
        assert log[-S.NALLOC - 1:] == ["s"] + frees(log), (j, log)  # the drain, then nothing but the frees


@pytest.mark.parametrize("kind", KINDS)
def test_success_path_synchronizes_once(kind):
    (rc, log), = S.run(["call -1 -1"], kind)
    assert rc == 0
    assert log == (["a%d" % i for i in range(S.NALLOC)] + ["o%d" % i for i in range(S.NOPS)] + ["s"] +
                   ["f%d" % i for i in range(S.NALLOC)])


@pytest.mark.parametrize("kind", KINDS)
def test_release_keeps_the_buffer(kind):
    (rc, log), (rc2, log2) = S.run(["release", "commit"], kind)
    assert rc == 0 and log == ["a0", "a1", "a2", "o0", "s", "f0", "f2"]
    # a buffer committed before anything was enqueued: nothing to drain, nothing to free
    assert rc2 == 0 and log2 == ["a0"]


@pytest.mark.parametrize("kind", KINDS)
def test_work_after_a_synchronize_is_drained_again(kind):
    (rc, log), = S.run(["rearm"], kind)
    assert rc == -S.BGV_E_DEVICE
    assert log == ["a0", "a1", "o0", "s", "o1", "y2", "s", "f0", "f1"]


@pytest.mark.parametrize("kind", KINDS)
def test_idle_scope_makes_no_policy_call(kind):
    (rc, log), = S.run(["idle"], kind)
    assert rc == 0 and log == []


@pytest.mark.parametrize("kind", KINDS)
def test_guard_without_buffers_drains_once(kind):
    (rc, log), (rc2, log2) = S.run(["guard 0", "guard 1"], kind)
    assert rc == 0 and log == ["o0", "o1", "s"]
    assert rc2 == -S.BGV_E_DEVICE and log2 == ["o0", "y1", "s"]

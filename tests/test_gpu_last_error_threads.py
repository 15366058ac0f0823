"""gm_last_error is per thread (include/geomesa_hip.h: "one gm_ctx per thread"; g_last_error in gm_ctx.hip is
thread_local): the text one thread reads is not changed by the argument errors another thread provokes.

Every call here is made with a NULL context and NULL or zero arguments.  Such a call returns GM_E_INVALID and sets
the text before the entry touches the device (density_check, freq_check, gm_density_sparse's first test), so the
module enqueues nothing, uses no stream and no context, and can run on its own.
"""
import ctypes
import threading

import pytest

from geomesa_amd import _lib

pytestmark = pytest.mark.gpu

# entries that name themselves in the text of a NULL-context error, so every call leaves a different text
LOUD = ["gm_density_points", "gm_density_arrow", "gm_density_lines", "gm_z3_frequency", "gm_frequency_points",
        "gm_cms_estimate"]
QUIET = "gm_density_sparse"
STEP_S = 10.0       # a thread that waits this long at a barrier has lost its partner
JOIN_S = 30.0


def provoke(lib, name):
    """The entry with a NULL context and every other argument NULL or zero: (return code, this thread's text)."""
    args = [None if a is ctypes.c_void_p else 0 for a in _lib.SIGNATURES[name][1]]
    rc = getattr(lib, name)(*args)
    return rc, lib.gm_last_error().decode(errors="replace")


def test_an_argument_error_on_one_thread_leaves_the_other_threads_text(gpu):
    lib = gpu.lib
    rc, mine = provoke(lib, "gm_bin_sort")
    assert rc == _lib.GM_E_INVALID and "gm_bin_sort" in mine
    step = threading.Barrier(2)
    seen = {"loud": [], "before": [], "after": []}
    failures = []

    def guarded(body):
        def run():
            try:
                body()
            except BaseException as e:      # a failed assertion or a broken barrier: reported by the test
                failures.append(e)
                step.abort()
        return threading.Thread(target=run, daemon=True)

    def quiet():
        rc, own = provoke(lib, QUIET)
        assert rc == _lib.GM_E_INVALID and QUIET in own
        seen["own"] = own
        for _ in LOUD:
            seen["before"].append(lib.gm_last_error().decode(errors="replace"))
            step.wait(STEP_S)       # the other thread provokes its error between these two waits
            step.wait(STEP_S)
            seen["after"].append(lib.gm_last_error().decode(errors="replace"))

    def loud():
        for name in LOUD:
            step.wait(STEP_S)
            rc, text = provoke(lib, name)
            assert rc == _lib.GM_E_INVALID and name in text, (name, rc, text)
            assert lib.gm_last_error().decode(errors="replace") == text     # read again between calls: it stays
            seen["loud"].append(text)
            step.wait(STEP_S)

    threads = [guarded(quiet), guarded(loud)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "a thread is still running"
    assert not failures, failures
    assert len(set(seen["loud"])) == len(LOUD)                       # several different texts were provoked
    assert seen["before"] == [seen["own"]] * len(LOUD) == seen["after"]
    assert seen["own"] not in seen["loud"]
    assert lib.gm_last_error().decode(errors="replace") == mine      # nor did either thread change this one's

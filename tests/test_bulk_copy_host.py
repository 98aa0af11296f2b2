"""Host suite: the chunk protocol of the staged host <-> device copies (csrc/figh_bulk_copy.h: two staging buffers, copy threads,
per-chunk completion counters, the `go` word) without a device.  tools/bulk_copy_host.cpp drives the header with a fake
transport -- one engine thread as the stream, a host array as device memory, events that complete when the engine reaches
them, seeded jitter in the engine and in the slice copies -- whose own checks (no slice copy on a staging buffer the engine
uses, every byte of a chunk copied exactly once, every chunk at its own offset, destination == source byte for byte, guard
bytes untouched) need no sanitizer.  The program is compiled with the host compiler alone ($CXX or c++), once plainly and
once under ThreadSanitizer, as an executable of its own: nothing is preloaded and nothing touches a GPU.

Cases (in the program): chunks of 16 and 3 pages, 1 ... 8 threads, both directions, byte counts 1, chunk - 1, chunk,
chunk + 1, two chunks, two chunks + 1, three chunks, five chunks and a ragged tail, two jitter seeds each; last chunks of
nt * 4096 * m + r bytes for every 0 < r < nt, m = 1, 2 (the sizes at which the share floor(n / nt) rounded up to a page left r
bytes to nobody; nt = 8, m = 2 does not fit a 16-page chunk and runs with 32 pages); bulk_slice itself for every nt and every
n up to 3 * 8 * 4096 + 8; and every transport operation of a five-chunk copy failing in turn, both directions, 1, 3 and 8
threads.  The path "the copy threads could not be started" is not exercised: it needs std::thread's constructor to throw.

Time limits are hang guards, not performance bounds: twenty times what the finished program took on the machine it was
written on (plain build 0.4 s, ThreadSanitizer build 4.1 s, every planted transport under 1 s; compiling 1.3 s and 2.3 s), and not
under 60 s."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "bulk_copy_host.cpp")
COMPILE_TIMEOUT = 60
RUN_TIMEOUT = {"plain": 60, "tsan": 82}
TSAN_FLAGS = ["-O1", "-g", "-fsanitize=thread", "-pthread"]

# a race-free program with a thread: can this host build and start ThreadSanitizer programs at all?
TSAN_PROBE = """
#include <mutex>
#include <thread>
int main() {
    std::mutex m;
    int x = 0;
    std::thread t([&] { std::lock_guard<std::mutex> l(m); ++x; });
    { std::lock_guard<std::mutex> l(m); ++x; }
    t.join();
    return x == 2 ? 0 : 1;
}
"""


def _cxx():
    cxx = shutil.which(os.environ.get("CXX", "c++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    return cxx


def _compile(cxx, flags, exe):
    subprocess.run([cxx, "-std=c++17"] + flags + ["-I" + os.path.join(ROOT, "figaroh_plus_amd", "csrc"), SOURCE, "-o", exe],
                   check=True, timeout=COMPILE_TIMEOUT)
    return exe


def _run(exe, what, build):
    """The program's exit status, stdout and stderr; a hang ends as subprocess.TimeoutExpired, a failure of the test."""
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=RUN_TIMEOUT[build])
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def plain_exe(tmp_path_factory):
    return _compile(_cxx(), ["-O2", "-pthread"], str(tmp_path_factory.mktemp("bulk_plain") / "bulk_copy_host"))


@pytest.fixture(scope="module")
def tsan_exe(tmp_path_factory):
    cxx = _cxx()
    d = tmp_path_factory.mktemp("bulk_tsan")
    probe_src, probe = str(d / "probe.cpp"), str(d / "probe")
    with open(probe_src, "w") as f:
        f.write(TSAN_PROBE)
    try:
        built = subprocess.run([cxx, "-std=c++17"] + TSAN_FLAGS + [probe_src, "-o", probe], capture_output=True, text=True,
                               timeout=COMPILE_TIMEOUT)
        ran = subprocess.run([probe], capture_output=True, text=True, timeout=60) if built.returncode == 0 else None
    except (OSError, subprocess.TimeoutExpired) as e:
        built, ran = None, None
        why = repr(e)
    else:
        why = (built.stderr if ran is None else "exit status %d: %s" % (ran.returncode, ran.stderr))[-400:]
    if ran is None or ran.returncode != 0:
        print("ThreadSanitizer probe failed:", why)
        pytest.skip("this host cannot build or start a race-free ThreadSanitizer probe: " + why)
    return _compile(cxx, TSAN_FLAGS, str(d / "bulk_copy_host_tsan"))


def test_plain_build_all_cases_pass(plain_exe):
    rc, out, err = _run(plain_exe, "all", "plain")
    print(out[-2000:], err[-2000:])
    assert rc == 0
    last = out.strip().splitlines()[-1].split()  # "bulk_copy_host: <runs> runs, <failed> failed"
    assert last[0] == "bulk_copy_host:" and int(last[1]) > 900 and int(last[3]) == 0
    assert "FAIL" not in out


@pytest.mark.parametrize("plant, every_run", [("plant-early-wait", False), ("plant-misroute", True), ("plant-drop-byte", True)])
def test_plain_build_detects_planted_transports(plain_exe, plant, every_run):
    """The fake transport's checks detect, in the plain build: an event wait that returns before the engine has reached the
    event (the engine is made late; a copy thread that is later still reads good data, so not every run must show it), a chunk
    routed to the other staging buffer and a slice that loses its last byte (both deterministic: every run, both directions)."""
    rc, out, err = _run(plain_exe, plant, "plain")
    print(out[-3000:], err[-2000:])
    assert rc == 1
    last = out.strip().splitlines()[-1].split()  # "... planted transport detected in <k> of <n> runs"
    detected, total = int(last[-4]), int(last[-2])
    assert total == 12 and detected >= 1
    assert any(l.startswith("detected d2h") for l in out.splitlines()) and any(l.startswith("detected h2d") for l in out.splitlines())
    if every_run:
        assert detected == total and "NOT DETECTED" not in out


def test_tsan_build_all_cases_pass_without_reports(tsan_exe):
    rc, out, err = _run(tsan_exe, "all", "tsan")
    print(out[-2000:], err[-4000:])
    assert rc == 0
    assert "ThreadSanitizer" not in err and "ThreadSanitizer" not in out
    last = out.strip().splitlines()[-1].split()
    assert int(last[1]) > 900 and int(last[3]) == 0


def test_tsan_build_reports_the_race_of_an_early_event_wait(tsan_exe):
    """With an event wait that orders nothing, ThreadSanitizer reports the race between the engine's write of a staging buffer and
    a copy thread's read of it (or, host -> device, the engine's read and the thread's write): the fake's waits are what orders
    the two, as hipEventSynchronize does in the product."""
    rc, out, err = _run(tsan_exe, "plant-early-wait", "tsan")
    print(out[-2000:], err[-6000:])
    assert rc != 0
    reports = err.split("WARNING: ThreadSanitizer: data race")[1:]
    assert reports
    # a report names its two threads (the program names them): one is the engine, the other a copy thread, and the
    # access is a memcpy of each
    assert any("'dma_engine'" in r and "'copy_worker'" in r and r.count("memcpy") >= 2 for r in reports)

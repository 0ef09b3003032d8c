"""The one place under tests/ that starts PE processes: launch().

  one deadline     `timeout` covers the whole job, counted from the first start
  output in files  each PE writes stdout and stderr (merged) to a file of its own,
                   read after the exit: no PE can stall on a full pipe
  all reaped       at the deadline, and on any exception on the way, every process
                   still running is killed and all are waited for
  no early kill    a PE that exits non-zero does not end its peers: tests assert that
                   those end by themselves, with the library's "aborting" message
  nothing else     it sets the PE identity, SHMEM_DEVICE or SHMEM_BOOTSTRAP_ONLY and the
                   hardware-queue policy; every other setting stays with its test
"""
import importlib.machinery
import importlib.util
import json
import os
import pathlib
import subprocess
import tempfile
import time
import uuid

HERE = os.path.dirname(os.path.abspath(__file__))
TAIL = 3000      # characters of a PE's output quoted in a failure message


def oshrun_module():
    """tools/oshrun (it has no .py suffix) as a module"""
    loader = importlib.machinery.SourceFileLoader("oshrun", os.path.join(os.path.dirname(HERE), "tools", "oshrun"))
    mod = importlib.util.module_from_spec(importlib.util.spec_from_loader("oshrun", loader))
    loader.exec_module(mod)
    return mod


class JobTimeout(AssertionError):
    """The job passed its deadline; every process was killed and reaped."""


def _record(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    try:
        return json.loads(lines[-1]) if lines else None
    except ValueError:
        return None


class Job:
    """Per PE `rc`, `out` and `record` (the last output line that starts with
    '{', parsed as JSON, or None); `started` (time.time() at the first start)
    and `elapsed` (seconds from the first start to the last exit)."""

    def __init__(self, rc, out, started, elapsed):
        self.rc, self.out, self.record = rc, out, [_record(o) for o in out]
        self.started, self.elapsed = started, elapsed

    def ok(self):
        for pe, (rc, out) in enumerate(zip(self.rc, self.out)):
            assert rc == 0, f"PE {pe} exited {rc}:\n{out[-TAIL:]}"
        return self

    def records(self):
        for pe, (rec, out) in enumerate(zip(self.ok().record, self.out)):
            assert rec is not None, f"PE {pe} printed no JSON record:\n{out[-TAIL:]}"
        return self.record


def launch(npes, argv, *, gpu, timeout, env=None, per_pe_env=None, identity=True):
    """Run `argv` as `npes` PE processes: the Job once all have exited, whatever their
    statuses, or JobTimeout. Environment, later entries winning: this process's; with
    `identity` SHMEM_NPES, a fresh SHMEM_JOB_ID and SHMEM_PE; SHMEM_DEVICE=0 and
    the queue policy (`gpu`) or SHMEM_BOOTSTRAP_ONLY=1; `env`; `per_pe_env[pe]`."""
    base = dict(os.environ)
    if identity:
        base.update(SHMEM_NPES=str(npes), SHMEM_JOB_ID=uuid.uuid4().hex[:12])
    if gpu:
        base["SHMEM_DEVICE"] = "0"
        # PEs sharing the one test GPU keep the job at 16 hardware queues, as under tools/oshrun
        base.update(oshrun_module().hw_queue_env(npes, True, base))
    else:
        base["SHMEM_BOOTSTRAP_ONLY"] = "1"
    base.update(env or {})
    procs, started, t0 = [], time.time(), time.monotonic()
    with tempfile.TemporaryDirectory(prefix="pes-") as logdir:
        try:
            for pe in range(npes):
                e = dict(base, SHMEM_PE=str(pe)) if identity else dict(base)
                e.update((per_pe_env or {}).get(pe, {}))
                with open(os.path.join(logdir, str(pe)), "wb") as f:
                    procs.append(subprocess.Popen(argv, env=e, stdout=f, stderr=subprocess.STDOUT))
            rc = []
            for p in procs:
                try:
                    rc.append(p.wait(timeout=max(0.0, t0 + timeout - time.monotonic())))
                except subprocess.TimeoutExpired:
                    rc.append(None)      # still running at the deadline
            elapsed = time.monotonic() - t0
        finally:
            for p in procs:
                p.kill()         # a process that has exited is left alone
            for p in procs:
                p.wait()
        out = [pathlib.Path(logdir, str(pe)).read_text(errors="replace") for pe in range(npes)]
    if None in rc:
        raise JobTimeout(f"the {npes}-PE job passed its deadline of {timeout} s\n" + "\n".join(
            f"PE {pe} " + ("killed at the deadline" if r is None else f"exited {r}") + f":\n{o[-TAIL:]}"
            for pe, (r, o) in enumerate(zip(rc, out))))
    return Job(rc, out, started, elapsed)

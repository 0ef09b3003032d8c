"""CPU: the PE launcher itself (tests/_pes.py), on `python -c` children that never load the library."""
import os
import subprocess
import sys
import time

import pytest

import _pes
from _pes import JobTimeout, launch

PE = "import os, sys, time\npe = int(os.environ.get('SHMEM_PE', -1))\n"
ENV = "print(*[os.environ.get(k, '-') for k in ('SHMEM_PE', 'SHMEM_NPES', 'SHMEM_JOB_ID', 'X_BOTH', 'X_ENV')])\n"
GPU = "print(*[os.environ.get(k) for k in ('SHMEM_DEVICE', 'SHMEM_BOOTSTRAP_ONLY', 'GPU_MAX_HW_QUEUES')])"


def run(npes, code, timeout=30, gpu=False, **kw):
    return launch(npes, [sys.executable, "-c", PE + code], gpu=gpu, timeout=timeout, **kw)


@pytest.mark.parametrize("writer", [0, 1])
def test_full_pipe(tmp_path, writer):
    """One PE prints 1 MiB, far more than a pipe holds, and only then lets its peer exit: a launcher
    that drains the PEs' pipes one at a time never ends when the peer comes first; this one does."""
    flag = str(tmp_path / "flag")
    job = run(2, f"if pe == {writer}:\n    sys.stdout.write('x' * (1 << 20)); sys.stdout.flush(); open({flag!r}, 'w')\n"
                 f"while not os.path.exists({flag!r}): time.sleep(0.01)\n").ok()
    assert job.elapsed < 15.0, job.elapsed
    assert len(job.out[writer]) == 1 << 20 and job.out[1 - writer] == ""


def test_deadline_kills_every_pe_and_keeps_the_output():
    t0 = time.monotonic()
    with pytest.raises(JobTimeout) as e:
        run(2, "print('MARK', pe, os.getpid(), flush=True)\nif pe == 1: time.sleep(60)\nsys.exit(4)", timeout=1)
    msg = str(e.value)
    assert time.monotonic() - t0 < 10.0 and isinstance(e.value, AssertionError)
    assert "PE 0 exited 4:" in msg and "PE 1 killed at the deadline:" in msg, msg
    marks = [ln.split() for ln in msg.splitlines() if ln.startswith("MARK ")]
    assert [m[1] for m in marks] == ["0", "1"], msg
    for m in marks:
        with pytest.raises(ProcessLookupError):
            os.kill(int(m[2]), 0)


def test_exit_codes_are_reported_and_nobody_is_killed_early():
    job = run(3, "if pe == 1: sys.exit(3)\n"
                 "if pe == 2: time.sleep(0.5)\n"          # still running when PE 1 has failed
                 "print('last line of', pe)")
    assert job.rc == [0, 3, 0] and job.out[2] == "last line of 2\n"
    with pytest.raises(AssertionError, match="PE 1 exited 3:"):
        job.ok()


def test_environment_layers(monkeypatch):
    monkeypatch.setenv("X_ENV", "inherited")
    ids = []
    for _ in range(2):
        job = run(3, ENV, env={"X_BOTH": "env", "X_ENV": "env"}, per_pe_env={1: {"X_BOTH": "pe1"}}).ok()
        rows = [o.split() for o in job.out]
        assert [r[:2] for r in rows] == [[str(pe), "3"] for pe in range(3)]
        assert len({r[2] for r in rows}) == 1 and len(rows[0][2]) == 12      # one job id for the job
        assert [r[3:] for r in rows] == [["env", "env"], ["pe1", "env"], ["env", "env"]]
        ids.append(rows[0][2])
    assert ids[0] != ids[1]
    # the site's env wins over the launcher's own variables, per_pe_env over both
    job = run(2, ENV + GPU, env={"SHMEM_BOOTSTRAP_ONLY": "0", "SHMEM_NPES": "7"},
              per_pe_env={1: {"SHMEM_PE": "5", "SHMEM_NPES": "9"}}).ok()
    assert [o.split()[:2] for o in job.out] == [["0", "7"], ["5", "9"]]
    assert [o.split()[-2] for o in job.out] == ["0", "0"]
    # identity=False: none of the three, also not inherited ones
    for k in ("SHMEM_PE", "SHMEM_NPES", "SHMEM_JOB_ID"):
        monkeypatch.delenv(k, raising=False)
    job = run(2, ENV + GPU, per_pe_env={r: {"X_BOTH": str(r)} for r in range(2)}, identity=False).ok()
    assert [o.split()[:4] for o in job.out] == [["-", "-", "-", "0"], ["-", "-", "-", "1"]]
    assert [o.split()[-2] for o in job.out] == ["1", "1"]                    # SHMEM_BOOTSTRAP_ONLY
    # gpu=True: the device, and tools/oshrun's policy before the site's env goes over it (no child touches a GPU)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    monkeypatch.delenv("SHMEM_KEEP_HW_QUEUES", raising=False)
    monkeypatch.delenv("SHMEM_BOOTSTRAP_ONLY", raising=False)
    assert run(4, GPU, gpu=True).out == ["0 None 4\n"] * 4
    assert run(8, GPU, gpu=True).out == ["0 None 2\n"] * 8
    assert run(8, GPU, gpu=True, env={"GPU_MAX_HW_QUEUES": "3"}).out == ["0 None 3\n"] * 8


def test_record_is_the_last_brace_line():
    job = run(3, "if pe == 0: print('{\"a\": 1}\\nnoise\\n{\"a\": 2, \"b\": [3]}\\ntrailing } text')\n"
                 "if pe == 1: print('no record here\\n {\"indented\": 1}')\n"
                 "if pe == 2: print('{\"a\": 1}\\n{not json')\n").ok()
    assert job.record == [{"a": 2, "b": [3]}, None, None]
    with pytest.raises(AssertionError, match="PE 1 printed no JSON record"):
        job.records()


def test_a_failed_start_reaps_the_pes_already_started(monkeypatch):
    started, real = [], subprocess.Popen

    def popen(argv, **kw):
        if len(started) == 2:
            raise FileNotFoundError("no such executable")
        started.append(real(argv, **kw))
        return started[-1]

    monkeypatch.setattr(_pes.subprocess, "Popen", popen)
    t0 = time.monotonic()
    with pytest.raises(FileNotFoundError):
        run(3, "time.sleep(60)")
    assert time.monotonic() - t0 < 10.0 and len(started) == 2
    for p in started:
        with pytest.raises(ProcessLookupError):
            os.kill(p.pid, 0)

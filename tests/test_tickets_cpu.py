"""The ticket protocol of the single stand-by launch (sdf_tools_amd/csrc/sdfgpu_tickets.hpp), executed on the CPU."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "tsan"])
def test_ticket_protocol_completes_with_fewer_workers_than_workgroups(sanitize):
    """k_envelope_standby runs the stand-by y sweep and the x sweep that needs ALL of it from one plain launch: workgroups claim
    tiles by ticket, y tiles first, and an x tile waits until every y tile has arrived.  tests/ticket_harness.cpp runs the header's
    claim / arrive / wait -- the very functions the kernel calls -- with G logical workgroups on R = 1, 2, 3 < G worker threads, a
    worker starting its next workgroup only when the current one has returned: every run completes, every ticket runs once, and
    every x tile starts after the last y tile and reads what all of them wrote.  Built plain and with -fsanitize=thread: the y
    tiles' words are plain memory."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tests = os.path.join(root, "tests")
    exe = os.path.join(tests, "ticket_harness_tsan" if sanitize else "ticket_harness")
    san = ["-fsanitize=thread", "-g", "-O1"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread"] + san + [os.path.join(tests, "ticket_harness.cpp"), "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:exitcode=66")
    r = subprocess.run([exe, "3", "6" if sanitize else "20"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr and "ticket protocol OK" in r.stdout, r.stdout + r.stderr[-3000:]

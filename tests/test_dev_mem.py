"""The engine's owner of device memory (gpudrive_lab_amd/csrc/dev_mem.hpp) on the host: tests/dev_mem_host.cpp links it
against an allocator over malloc that records live blocks, counts frees of unknown blocks and can make the n-th
allocation throw.  Moves, reserve within and beyond the capacity, a failed reserve, a vector of owners that unwinds."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dev_mem_on_a_host_allocator(tmp_path):
    exe = str(tmp_path / "dev_mem_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "dev_mem_host.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout

"""The chunk arithmetic of the index movers (IxChunks, mapquik_amd/csrc/mq_ix_chunks.hpp) on the host: tests/cpp/ix_chunks_test.cc built with
ASan + UBSan as a stand-alone program and run; and the one place that reads the MQ_IX_IO_CHUNK test hook spells it as the GPU test
(tests/test_gpu_index_io_chunks.py, which cannot see from outside whether the hook took effect) sets it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ix_chunks(tmp_path):
    exe = str(tmp_path / "ix_chunks_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "ix_chunks_test.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ix_chunks ok" in r.stdout, r.stdout + r.stderr


def test_hook_name_is_the_one_the_gpu_test_sets():
    io = open(os.path.join(ROOT, "mapquik_amd", "csrc", "mq_capi_index_io.hpp")).read()
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_index_io_chunks.py")).read()
    read = re.findall(r'env_int\("(MQ_IX_IO_CHUNK)", 64 << 20\)', io)
    assert read == ["MQ_IX_IO_CHUNK"], read  # read once, with the product's 64 MB as the default
    assert 'HOOK, CHUNK = "MQ_IX_IO_CHUNK", "96"' in gpu
    assert len(re.findall(r"\bIxChunks\(", io)) == 1  # ... and every chunk loop gets its chunks from that one place

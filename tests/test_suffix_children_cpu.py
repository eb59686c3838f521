"""The suffix table's deepest level as child lists (fmx_device.hpp: DevIndex.suffix_child_rows) on the host: the device header's
lookup and list-building functions in a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_child_lists_answer_every_string_of_the_deepest_level_and_are_sanitizer_clean(tmp_path):
    """tests/cpp/san_suffix_children.cpp: hashed levels to D, level D + 1 as child lists, on a synthetic log (D = 2, 3) and on 12
    random symbols over 2^20 - 1 and 2^20 characters (D = 4; one of the two has strings whose search raises a status).  Every
    string of 2 .. D + 1 characters that occurs looks up to the interval of the loop (and holds as many rows as the string has
    occurrences) or, where the loop raises a status, misses; 10,000 absent strings miss, half of them with an occurring parent;
    lists grown with every third string left out flag the gaps, miss the strings left out and still answer the others."""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "index4j_amd", "csrc")
    exe = str(tmp_path / "san_suffix_children")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + csrc, "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "san_suffix_children.cpp")]
    cmd += [os.path.join(csrc, f) for f in ("fmx_build.cpp", "fmx_serial.cpp", "fmx_blob.cpp", "fmx_synth.cpp")]
    cmd += ["-lpthread", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-6000:]
    assert r.stdout.count(" ok: ") == 4, r.stdout[-3000:]
    assert "FAILED" not in r.stdout

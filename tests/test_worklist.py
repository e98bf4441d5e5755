"""The work list between the staged kernels and the direct-gather kernel (envutil_amd/csrc/eu_worklist.h) is plain
C++ on the host: a program replays the writers' appends - the list a tile id hashes to, that list's next slot, the
index the id is stored at - for every launch size from 1 to 16384 tiles, for 98304, 786432 (the headline) and 2^20
tiles and for the largest launch the staged path accepts, with every tile listed and with every third / seventh
listed, and checks every index against the buffer eu_render4_worklist_ints() asks for. The capacity must hold
(slack >= 0) without simply doubling the buffer: slack < 2 * EU4_SHARDS + ntiles / 64.

With the capacity sized for `id % 1024` lists (ceil(ntiles / 1024) entries per list, the rule until this header
existed) the same program reports a first failure at 611 tiles - ids 0 and 610 share list 0 - and from 1024 tiles on
a shortfall of a thousand ints and more:
    FAILED: every tile listed: ntiles = 611: fullest list 2, highest index 17664, capacity 17664 ints: 1 ints past the end
    slack 1024 -1005
    slack 4096 -1016
    slack 786432 -2304
    FAILED: every third tile listed: ntiles = 991: fullest list 2, highest index 18538, capacity 17664 ints: 875 ints past the end
and with the counted capacity
    slack 1024 19
    slack 4096 8
    slack 786432 768
    ok: every tile listed, 2147483647 ids listed, 16388 sizes checked up to ntiles = 2147483647

The last size is what the test costs: the program replays 2^31 appends and the census behind the capacity hashes
the same 2^31 ids, about 7 s of one core together (every other size is done within 30 ms). It stays, because the
int limit is the one size at which the id, the slot and the capacity in ints all come near their types' ends."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "envutil_amd", "build", "worklist_demo")


def test_worklist_host_program():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "csrc", "worklist_demo.cc"), "-o", EXE])
    r = subprocess.run([EXE], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "all ok" in r.stdout
    shards = int(re.search(r"^shards (\d+)$", r.stdout, re.M).group(1))
    assert shards == 1024
    slack = {int(n): int(s) for n, s in re.findall(r"^slack (\d+) (-?\d+)$", r.stdout, re.M)}
    assert sorted(slack) == [1024, 4096, 786432]
    for ntiles, s in slack.items():
        assert 0 <= s < 2 * shards + ntiles // 64, (ntiles, s)
    # every sweep ran to its end
    assert len(re.findall(r"^ok: every (tile|third tile|seventh tile) listed", r.stdout, re.M)) == 3
    assert int(re.search(r"^largest launch (\d+) tiles$", r.stdout, re.M).group(1)) == 2 ** 31 - 1

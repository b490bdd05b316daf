"""The channels a retained step's written windows read, without a GPU: the compile-time tables
of gym-td_amd/csrc/td_obs_win.h (ObsWinTab: chan, dtab, ntab), printed by the host program
scripts/channel_needs_host.cpp, against a plain restatement of the windows:

    window k of a board at misalignment m covers the board's units [64 k - m, 64 k - m + 63];
    a channel is 25 (L / 10)^2 units; the board has 45 channels.

for L = 10, 20, 30 and both unit sizes (8 units of float32 or 16 of float16 per 128-B line).
A written window is written whole, so the channels needed are those of every window one of
whose dirty classes is dirty -- not the dirty classes' channels alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCH = 45
OD_STATIC, OD_LP, OD_TOWER, OD_COST, OD_ENEMY, OD_ALWAYS = 1, 2, 4, 8, 16, 32
SHAPES = [(L, upl) for L in (10, 20, 30) for upl in (8, 16)]


def dirty_class(ch):
    """td_retain_obs's classes, as DESIGN.md lists them."""
    if ch == 5:
        return OD_LP
    if ch <= 10:
        return OD_STATIC
    if ch in (11, 12, 13) or ch >= 41:
        return OD_ALWAYS
    if ch <= 20:
        return OD_TOWER
    if ch <= 24:
        return OD_COST
    return OD_ENEMY


def windows(L, upl):
    q = 25 * (L // 10) ** 2
    n4 = NCH * q
    return q, n4, (n4 + upl - 1 + 63) // 64


def chan(L, upl, m, k):
    q, n4, _ = windows(L, upl)
    mask = 0
    for u in range(64 * k - m, 64 * k - m + 64):
        if 0 <= u < n4:
            mask |= 1 << (u // q)
    return mask


def classes(mask):
    d = 0
    for c in range(NCH):
        if (mask >> c) & 1:
            d |= dirty_class(c)
    return d


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("chneeds") / "channel_needs_host")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "scripts", "channel_needs_host.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    t = {"shape": {}, "chan": {}, "dirty": {}, "need": {}}
    for ln in run.stdout.split("\n"):
        f = ln.split()
        if not f:
            continue
        if f[0] == "shape":
            t["shape"][(int(f[1]), int(f[2]))] = int(f[4])
        else:
            t[f[0]][tuple(int(v) for v in f[1:5])] = int(f[5], 16)
    return t


@pytest.mark.parametrize("L,upl", SHAPES)
def test_window_channels_and_classes(tables, L, upl):
    _, _, K = windows(L, upl)
    assert tables["shape"][(L, upl)] == K
    seen = 0
    for m in range(upl):
        union = 0
        for k in range(K):
            want = chan(L, upl, m, k)
            assert tables["chan"][(L, upl, m, k)] == want, ("chan", m, k)
            assert tables["dirty"][(L, upl, m, k)] == classes(want), ("dirty", m, k)
            union |= want
            seen += 1
        assert union == (1 << NCH) - 1  # the windows cover the board
    assert seen == upl * K == sum(1 for key in tables["chan"] if key[:2] == (L, upl))


@pytest.mark.parametrize("L,upl", SHAPES)
def test_needed_channels_of_every_dirty_set(tables, L, upl):
    _, _, K = windows(L, upl)
    for m in range(upl):
        for i in range(16):
            dirty = OD_ALWAYS | (i << 1)
            want = 0
            for k in range(K):
                c = chan(L, upl, m, k)
                if classes(c) & dirty:
                    want |= c
            got = tables["need"][(L, upl, m, i)]
            assert got == want, ("need", m, i, hex(got), hex(want))
            # never less than the dirty classes' own channels
            own = sum(1 << c for c in range(NCH) if dirty_class(c) & dirty)
            assert got & own == own


def test_the_two_cases_a_class_alone_would_miss(tables):
    """10x10 float32: window 5 of a board whose ALWAYS class alone is dirty holds tower planes;
    at misalignment 7 window 4 holds the last unit of channel 9 -- and at no other."""
    w5 = tables["chan"][(10, 8, 0, 5)]
    assert (w5 >> 13) & 1 and (w5 >> 14) & 1 and dirty_class(14) == OD_TOWER
    assert (tables["need"][(10, 8, 0, 0)] >> 14) & 1
    assert (tables["chan"][(10, 8, 7, 4)] >> 9) & 1
    for m in range(8):
        for i in range(16):
            assert (tables["need"][(10, 8, m, i)] >> 9) & 1 == (1 if m == 7 else 0), (m, i)

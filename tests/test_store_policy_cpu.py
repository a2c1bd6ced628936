"""The host's store policy (stratego_env_amd/csrc/sgx_store_policy.h: which share of a multi-step launch's observation lines leaves as plain
stores) WITHOUT a GPU: the header is compiled with the host compiler into a small program that prints the header's constants and, for
every shape on its standard input, the policy.  Regimes, monotonicity, whole sweeps and the budget arithmetic are checked against the
constants the header exports, not against literals."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, 'stratego_env_amd', 'csrc', 'sgx_store_policy.h')
OUT_DIR = os.path.join(ROOT, 'tests', '_build')
SRC = os.path.join(OUT_DIR, 'store_policy_probe.cpp')
EXE = os.path.join(OUT_DIR, 'store_policy_probe')

PROGRAM = r'''
#include <stdio.h>
#include "sgx_store_policy.h"
int main() {
    printf("%lld %lld %d %d %d %d\n", (long long)SGX_CACHE_FIT_BYTES, (long long)SGX_PLAIN_BUDGET_BYTES, SGX_STORE_LINE_BYTES, SGX_STORE_SWEEP_LINES,
           SGX_RESULT_BYTES, SGX_STORE_SPLIT_DEFAULT);
    long long cus, wg, gpw, games, sets, obs, fobs, mask, budget, split;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &cus, &wg, &gpw, &games, &sets, &obs, &fobs, &mask, &budget, &split) == 10) {
        sgx_store_shape s;
        s.cus = (int32_t)cus; s.wg_per_cu = (int32_t)wg; s.games_per_wg = (int32_t)gpw; s.games = games; s.sets = (int32_t)sets;
        s.obs_bytes = obs; s.fobs_bytes = fobs; s.mask_bytes = mask; s.budget = budget; s.split = (int32_t)split;
        const sgx_store_policy p = sgx_store_policy_multi_step(&s);
        printf("%d %d %d %lld %lld %d %d\n", p.nt_stores, p.plain_lines, p.fobs_plain_lines, (long long)sgx_store_resident_games(&s),
               (long long)sgx_store_rewrite_set(&s), sgx_store_max_plain_lines(obs), sgx_store_max_plain_lines(fobs));
    }
    return 0;
}
'''

# Barrage, 10x10: float32 [10,10,67] partial and [10,10,79] full observation, uint8 [10,10,37] mask
OBS, FOBS, MASK = 4 * 67 * 100, 4 * 79 * 100, 37 * 100
CUS, WG, GPW = 256, 3, 8          # MI355X; steps_kernel<10,10,0>: 3 resident workgroups of 8 waves, one game per wave


@pytest.fixture(scope='module')
def probe():
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip("no host C++ compiler: the store policy header cannot be compiled on its own")
    os.makedirs(OUT_DIR, exist_ok=True)
    if not os.path.exists(SRC) or open(SRC).read() != PROGRAM:
        with open(SRC, 'w') as f:
            f.write(PROGRAM)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call([cxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-I', os.path.dirname(HDR), SRC, '-o', EXE])

    def run(shapes):
        text = ''.join(' '.join(str(int(x)) for x in s) + '\n' for s in shapes)
        lines = subprocess.run([EXE], input=text, capture_output=True, text=True, check=True).stdout.split('\n')
        consts = dict(zip(('cache_fit', 'budget', 'line', 'sweep_lines', 'result', 'split_default'), (int(x) for x in lines[0].split())))
        rows = [dict(zip(('nt', 'plain', 'fplain', 'resident', 'rewrite', 'max_plain', 'max_fplain'), (int(x) for x in ln.split()))) for ln in lines[1:] if ln]
        assert len(rows) == len(shapes)
        return consts, rows
    return run


def shape(budget, games=65536, sets=1, obs=OBS, fobs=0, mask=MASK, cus=CUS, wg=WG, gpw=GPW, split=1):
    return (cus, wg, gpw, games, sets, obs, fobs, mask, budget, split)


def test_regimes(probe):
    c, _ = probe([])
    b = c['budget']
    _, (ring3, in_place, ring9, traj64, small, both3) = probe([shape(b, sets=3), shape(b, sets=1), shape(b, sets=9), shape(b, sets=64),
                                                              shape(b, games=251, sets=3), shape(b, sets=3, fobs=FOBS)])
    # the headline: 65,536 Barrage games into a ring of three -- a split
    assert ring3['nt'] == 1 and 0 < ring3['plain'] < ring3['max_plain']
    assert ring3['resident'] == CUS * WG * GPW
    # the same games in place: what 6,144 resident games rewrite fits -- all plain
    assert in_place['nt'] == 0 and in_place['rewrite'] <= b
    # long rings and trajectory buffers: nothing left after mask and results, by arithmetic
    assert ring9['nt'] == 1 and ring9['plain'] == 0 and ring9['fplain'] == 0
    assert traj64['nt'] == 1 and traj64['plain'] == 0 and traj64['fplain'] == 0
    # a batch smaller than the resident games: the batch is what is rewritten
    assert small['resident'] == 251 and small['rewrite'] == 251 * 3 * (OBS + MASK + c['result']) and small['nt'] == 0
    # with the split switched off a rewrite set beyond the budget gets no plain share, one within it is all plain as before
    _, (off3, off1) = probe([shape(b, sets=3, split=0), shape(b, sets=1, split=0)])
    assert off3['nt'] == 1 and off3['plain'] == 0 and off3['fplain'] == 0 and off1['nt'] == 0
    # BOTH mode: the partial observation is served first
    assert both3['nt'] == 1 and both3['plain'] >= both3['fplain'] and (both3['fplain'] == 0 or both3['plain'] == both3['max_plain'])


def test_properties_and_budget_arithmetic(probe):
    c, _ = probe([])
    sweep = c['sweep_lines']
    shapes = []
    for budget in (c['budget'], c['budget'] // 2, 2 * c['budget'], 0):
        for fobs in (0, FOBS):
            for games in (1, 9, 251, 6144, 6145, 65536, 262144):
                for wg in (1, 2, 3, 4, 8):
                    for sets in (1, 2, 3, 4, 8, 9, 16, 64):
                        shapes.append(shape(budget, games=games, sets=sets, fobs=fobs, wg=wg))
    _, rows = probe(shapes)
    by_shape = dict(zip(shapes, rows))
    for s, r in by_shape.items():
        cus, wg, gpw, games, sets, obs, fobs, mask, budget, _ = s
        assert r['plain'] % sweep == 0 and r['fplain'] % sweep == 0, s              # whole sweeps
        assert 0 <= r['plain'] <= r['max_plain'] <= -(-obs // c['line']), s           # never more than the observation's lines
        assert 0 <= r['fplain'] <= r['max_fplain'] <= -(-fobs // c['line']), s
        assert r['resident'] == min(cus * wg * gpw, games), s
        assert r['rewrite'] == r['resident'] * sets * (obs + fobs + mask + c['result']), s
        assert (r['nt'] == 0) == (r['rewrite'] <= budget), s
        if r['nt']:          # mask + results + plain shares <= budget per resident game and set
            share = mask + c['result'] + (r['plain'] + r['fplain']) * c['line']
            assert r['plain'] + r['fplain'] == 0 or share * r['resident'] * sets <= budget, s
            assert r['fplain'] == 0 or r['plain'] == r['max_plain'], s               # the partial observation first
        # never more plain lines with more sets or more resident waves (nt = 0 counts as everything)
        total = (r['plain'] + r['fplain']) if r['nt'] else (r['max_plain'] + r['max_fplain'] + 1)
        for other in (shape(budget, games=games, sets=sets * 2 if sets < 64 else sets, fobs=fobs, wg=wg),
                      shape(budget, games=games, sets=sets, fobs=fobs, wg={1: 2, 2: 3, 3: 4, 4: 8, 8: 8}[wg])):
            if other in by_shape:
                o = by_shape[other]
                assert ((o['plain'] + o['fplain']) if o['nt'] else (o['max_plain'] + o['max_fplain'] + 1)) <= total, (s, other)


def test_constants(probe):
    c, _ = probe([])
    assert c['line'] == 128 and c['sweep_lines'] * c['line'] == 1024           # a sweep of emit_codes is 1 KiB of whole lines
    assert c['result'] == 12
    assert c['split_default'] in (0, 1)
    assert 0 < c['budget'] <= 256 * 1024 * 1024                                  # never more than the Infinity Cache itself

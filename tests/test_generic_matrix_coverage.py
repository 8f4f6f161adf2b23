"""The generic-kernel sweep (tests/test_gpu_generic_matrix.py) covers what adm_ms_generic.hip launches: tests/gen_matrix.py mirrors
its launch arithmetic, and this CPU test parses the sources -- GEN_E, ms_generic_threads, ms_generic_supported, red[], factor()'s
radix list and the __global__ kernels -- so that a change there fails here until the tables follow.  It asserts that the tables
reach every class of geometry and every run-time branch they name, and it runs the oracle alone (fp64 and fp32, no GPU) over
every case of the sweep: no slot band of a prediction or a probe gradient may be without signal, and the oracle's own fp32 run
may use at most a third of a whole-array bar -- a case that cannot meet that measures its data, not the kernel."""
import os
import re

import numpy as np
import pytest

from tests import gen_matrix as GM
from tests import ms_matrix as MM
from tests.test_gpu_generic_matrix import oracle_case, slot_sets
from tests.test_gpu_streamed_matrix import band_errors
from tests.test_kernel_matrix_coverage import _function_body
from tests.test_streamed_matrix_coverage import _read, c_int_function, constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = MM.GENERIC


def parsed():
    gen, hip, api = _read('adm_ms_gen.h'), _read('adm_ms_generic.hip'), _read('adm_api.hip')
    c = constants(gen, ['GEN_E'])
    # ms_generic_threads as a function of n (px = 1)
    nt = c_int_function(_function_body(hip, r'int\s+ms_generic_threads\s*\(\s*int\s+py\s*,\s*int\s+px\s*\)'), dict(c, px=1))
    return gen, hip, api, c, nt


def test_the_mirror_uses_the_source_constants():
    gen, hip, api, c, _ = parsed()
    assert GM.GEN_E == c['GEN_E']
    body = _function_body(hip, r'int\s+ms_generic_threads\s*\(\s*int\s+py\s*,\s*int\s+px\s*\)')
    m = re.search(r'int nt = \(\(n \+ GEN_E - 1\) / GEN_E \+ (\d+)\) / (\d+) \* (\d+);\s*if \(nt < (\d+)\) nt = (\d+);', body)
    assert m, body
    assert [int(v) for v in m.groups()] == [GM.NT_ROUND - 1, GM.NT_ROUND, GM.NT_ROUND, GM.NT_FLOOR, GM.NT_FLOOR]
    body = _function_body(hip, r'bool\s+ms_generic_supported\s*\(\s*int\s+py\s*,\s*int\s+px\s*\)')
    m = re.search(r'const size_t lds = \(\(size_t\)py \* px \+ px \+ py\) \* sizeof\(float2\) \+ (\d+);\s*'
                  r'return ms_generic_threads\(py, px\) <= (\d+) && lds <= ([\d*\s+-]+);', body)
    assert m, body
    assert (int(m.group(1)), int(m.group(2)), eval(m.group(3), {'__builtins__': {}})) == (GM.LDS_SLACK, GM.NT_CAP, GM.LDS_LIMIT)
    assert '160 * 1024 - 256' in m.group(3)
    # the launch: the same field + twiddle rows, the attribute at the same limit, the kernel's bound and its partial sums
    launch = _function_body(hip, r'hipError_t\s+ms_generic_launch\s*\(')
    assert 'const size_t lds = ((size_t)p.gen_py * p.gen_px + p.gen_px + p.gen_py) * sizeof(float2);' in launch
    assert 'hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256)' in launch
    assert re.search(r'__launch_bounds__\((\d+)\)\s+void\s+ms_generic_kernel', hip).group(1) == str(GM.NT_CAP)
    assert re.search(r'__shared__\s+float\s+red\[(\d+)\]', hip).group(1) == str(GM.RED_SLOTS)
    assert GM.RED_SLOTS == GM.NT_CAP // 64 == max(GM.WAVE_COUNTS)           # gen_block_sum walks nt >> 6 of them
    assert 'for (int w = 0; w < (nt >> 6); ++w) s += red[w];' in _function_body(gen, r'float\s+gen_block_sum\s*\(')
    # the slot rule and its guard
    kernel = _function_body(hip, r'void\s+ms_generic_kernel\s*\(')
    assert 'g.ne = (g.n + g.nt - 1) / g.nt;' in kernel
    assert len(re.findall(re.escape('const int i = g.tid + j * g.nt;'), kernel + gen)) == len(re.findall(re.escape('if (j < g.ne && i < g.n)'), kernel + gen)) == 6
    # factor(): the preferred radices, at most 8 of them, the leftover primes from 11 in steps of 2
    m = re.search(r'const\s+int\s+pref\[\]\s*=\s*\{([^}]*)\}', api)
    assert m and tuple(int(v) for v in m.group(1).split(',')) == GM.SM.PREF
    body = _function_body(api, r'auto\s+factor\s*=\s*\[\]\s*\(int n, int\* r\)')
    assert set(re.findall(r'cnt\s*<\s*(\d+)', body)) == {str(GM.SM.MAX_RADICES)}
    assert re.search(r'for\s*\(int q = 11;[^;]*;\s*q \+= 2\)', body)
    assert GM.factor is GM.SM.factor


def test_the_mirror_follows_ms_generic_threads_at_every_n():
    nt = parsed()[4]
    for n in range(1, GM.NT_CAP * GM.GEN_E + 1):
        t = nt(n)
        assert GM.threads(n, 1) == GM.threads(1, n) == t, n
        assert t % 64 == 0 and GM.NT_FLOOR <= t <= GM.NT_CAP and -(-n // t) <= GM.GEN_E, n
    assert nt(GM.NT_CAP * GM.GEN_E + 1) > GM.NT_CAP
    assert {GM.threads(n, 1) // 64 for n in range(1, GM.NT_CAP * GM.GEN_E + 1)} == set(GM.WAVE_COUNTS)
    assert [GM.threads(*s) for s in ((16, 16), (64, 64), (64, 65), (127, 129), (128, 128))] == [256, 256, 320, 1024, 1024]


def test_the_acceptance_edges():
    for s in GM.LDS_REFUSED:
        assert s[0] * s[1] == 16384 and GM.threads(*s) <= GM.NT_CAP and GM.lds_bytes(*s) > GM.LDS_LIMIT and not GM.supported(*s), s
    assert GM.supported(*GM.LDS_ACCEPTED) and GM.LDS_ACCEPTED in GM.SHAPES
    for s in MM.GENERIC_REFUSED:
        assert GM.threads(*s) > GM.NT_CAP and not GM.supported(*s), s          # refused by n > 16384
    assert all(GM.supported(*s) for s in GM.SHAPES) and all(GM.supported(*s) for s in MM.GENERIC_FIELDS)
    assert MM.GENERIC_REFUSED == [(129, 128), (128, 129), (16, 1040)]
    assert MM.GENERIC == dict(pred=5e-6, loss=3e-5, grad=2e-4, grad_abs=2e-5, probe_3x=False, shift=2e-4)


def test_slot_bands_tile_the_field():
    for s in GM.SHAPES:
        g, b = GM.geometry(*s), GM.slot_bands(*s)
        assert b[0][0] == 0 and b[-1][1] == g['n'] and len(b) == g['ne'] <= GM.GEN_E
        assert all(hi == lo2 for (_, hi), (lo2, _) in zip(b, b[1:])) and all(hi - lo == g['nt'] for lo, hi in b[:-1])
        assert b[-1][1] - b[-1][0] == g['last']
    assert GM.geometry(127, 129)['last'] == 1023 and GM.geometry(16, 17)['last'] == 16 and GM.geometry(33, 31)['last'] == 255
    g = GM.geometry(64, 65)
    assert (g['nt'], g['ne'], g['last']) == (320, 13, 320)
    assert GM.geometry(8, 1890)['radix_x'] == [2, 9, 3, 5, 7] and GM.geometry(11, 143)['radix_x'] == [11, 13]
    assert GM.geometry(3, 4096)['radix_x'] == [8, 8, 8, 8] and GM.geometry(8, 2039)['radix_x'] == [2039] and GM.geometry(1, 64)['radix_y'] == []


def test_every_class_is_reached():
    reached = {}
    for shape in GM.SHAPES:
        for c in GM.classes(*shape):
            reached.setdefault(c, []).append(shape)
    assert set(reached) <= set(GM.ALL_CLASSES), set(reached) - set(GM.ALL_CLASSES)
    missing = [c for c in GM.ALL_CLASSES if c not in reached]
    assert not missing, 'classes no entry of SHAPES reaches: %s' % missing
    assert set(reached['n_max_full']) >= {(128, 128), (8, 2048)} and (127, 129) in reached['n_max_ragged'] and (64, 64) in reached['ne_16_full_nt256']
    # every single-radix side on either axis; both orientations of every non-square field that carries an axis class
    for ax in (0, 1):
        assert {s[ax] for s in GM.SHAPES if GM.factor(s[ax]) == [s[ax]]} >= {2, 3, 5, 7}, ax
    rare = ('single_radix_2_3_5_7', 'leftover_two_primes', 'leftover_prime_large', 'passes_ge_5', 'four_passes_of_8', 'side_1')
    for s in GM.SHAPES:
        if s[0] != s[1] and any(c.rsplit('_', 1)[0] in rare for c in GM.classes(*s)):
            assert s[::-1] in GM.SHAPES, s
    assert (129, 127) in GM.SHAPES and (2048, 8) in GM.SHAPES
    assert all(kw['B'] >= 4 for kw in GM.SHAPES.values())         # (one position over each corner)
    # a square field of a tuned size reaches this kernel only when the plan is told so; no other field may ask for it
    for s, kw in GM.SHAPES.items():
        assert kw.get('generic', False) == (s[0] == s[1] and s[0] in MM.SIZES), s
    assert all(not (s[0] == s[1] and s[0] in MM.SIZES) for s in list(GM.SEQUENCE_SHAPES.values()) + GM.TRANSPOSED_PAIRS + [(127, 129)])


def test_every_sequence_is_filed_at_both_thread_counts():
    assert set(GM.SEQUENCE_SHAPES) == {'nt256', 'nt640'}
    a, b = (GM.geometry(*GM.SEQUENCE_SHAPES[k]) for k in ('nt256', 'nt640'))
    assert a['nt'] == GM.NT_FLOOR and b['nt'] > GM.NT_FLOOR and all(1 < g['last'] < g['nt'] and g['ne'] > 1 for g in (a, b))
    assert set(GM.SEQUENCE_CASES) == {(n, c) for n in GM.SEQUENCES for c in GM.SEQUENCE_SHAPES}
    reached = set().union(*(GM.features(n) for n in GM.SEQUENCES))
    assert reached == set(GM.REQUIRED_FEATURES), (reached ^ set(GM.REQUIRED_FEATURES))
    for n in GM.SEQUENCES:
        kw, flags = GM.sequence_kw(n)
        assert kw['B'] >= 4 and 'generic' not in kw and kw.get('pp') in (None, 'probes'), n
        if isinstance(kw.get('free_prop'), list):
            assert kw['B'] % len(kw['free_prop']) == 0, n
        assert not (flags and kw.get('pp')), n                    # (the flagged launches hand over one shared probe set)


def test_the_matrix_names_exactly_the_kernels_of_the_source():
    hip = parsed()[1]
    found = set(re.findall(r'__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', hip))
    assert len(re.findall(r'__global__', hip)) == len(found) == 1, sorted(found)
    assert found == set(GM.KERNELS), found ^ set(GM.KERNELS)
    for k, (module, tests) in GM.KERNELS.items():
        with open(os.path.join(ROOT, 'tests', module + '.py')) as f:
            text = f.read()
        for t in tests:
            assert re.search(r'^def %s\(' % t, text, re.M), (k, module, t)
    # the run-time branches the sequences are named after are still in the kernel
    for text in ('p.n_hfree > 1 ? (size_t)(b % p.n_hfree) * g.n : 0', 'if (p.det_inverse) gen_fft2<true>(g, p, v); else gen_fft2<false>(g, p, v);',
                 'if (!do_grad) return;', 'if (p.pred) p.pred[di] = mag;', 'if (p.grad_probe) {', 'if (m > 0) { const float2 o = *gq;',
                 'float2* dq = p.det + ((size_t)b * M + m) * row;', '(ky + g.Py / 2) % g.Py', 'p.det_weight && p.det_weight[my * g.Px + mx] == 0.f'):
        assert text in hip, text


# ------------------------------------------------------------------------------------------- the cases on the oracle alone
def oracle_conditions(case, what):
    """No slot band of any position's prediction or any mode's probe gradient without signal; the fp32 oracle within a third of
    every whole-array bar."""
    kw = case['kw']
    shape, far = kw['shape'], kw['free_prop'] == 'inf'
    r32 = lambda k: MM.rel(case[k + '_32'], case[k + '_o'])
    assert r32('pred') < BARS['pred'] / 3, (what, 'pred', r32('pred'))
    assert abs(case['loss_32'] - case['loss_o']) < BARS['loss'] / 3 * abs(case['loss_o']), (what, 'loss')
    assert r32('grad') < BARS['grad'] / 3, (what, 'grad', r32('grad'))
    names = (('pred', far),) if kw['pp'] == 'probes' else (('pred', far), ('gprobe', False))
    if kw['pp'] != 'probes':
        assert r32('gprobe') < BARS['grad'] / 3, (what, 'gprobe', r32('gprobe'))
    for name, shifted in names:
        for k in range(len(case[name + '_o'])):
            (e, e32, judged), = band_errors(case[name + '_32'][k], case[name + '_o'][k], case[name + '_32'][k], shape, shifted, slot_sets(shape))
            assert judged.all(), (what, name, k, 'slot bands without signal', np.flatnonzero(~judged))
            assert np.isfinite(e32).all() and e32.max() < (BARS['pred'] if name == 'pred' else BARS['grad']) / 3, (what, name, k, e32.max())


@pytest.mark.parametrize('shape', list(GM.SHAPES), ids=lambda s: '%dx%d' % s)
def test_shape_cases_on_the_oracle_alone(shape):
    cl = GM.classes(*shape)
    assert len(cl & {'waves_%d' % w for w in GM.WAVE_COUNTS}) == 1, cl
    oracle_conditions(oracle_case(shape, **GM.SHAPES[shape]), shape)


@pytest.mark.parametrize('name,cls', GM.SEQUENCE_CASES)
def test_sequence_cases_on_the_oracle_alone(name, cls):
    oracle_conditions(oracle_case(GM.SEQUENCE_SHAPES[cls], **GM.sequence_kw(name)[0]), (name, cls))


def test_other_cases_on_the_oracle_alone():
    for shape in GM.TRANSPOSED_PAIRS:
        oracle_conditions(oracle_case(shape, S=3, B=5, n_modes=2, seed=7), shape)
    oracle_conditions(oracle_case((127, 129), S=3, B=5, n_modes=3), '127x129')
    for n in GM.SEQUENCES:
        kw, flags = GM.sequence_kw(n)
        if flags:
            oracle_conditions(oracle_case((127, 129), **kw), (n, '127x129'))

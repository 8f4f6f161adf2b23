"""The launch geometries of the any-size multislice kernel (ms_generic_kernel of adm_ms_generic.hip, helpers in adm_ms_gen.h)
and the fields that reach each of them (test infrastructure only).

The kernel is compiled once and takes everything at run time, so its classes are launch geometries and flag combinations, not
instantiations.  ``geometry`` mirrors ms_generic_threads / ms_generic_supported, the slot rule of the kernel (element
``i = tid + j * nt`` lives in register slot ``j``) and, through st_matrix.factor, the radix lists of plan_create; ``classes``
names what a field exercises of them.  ``SHAPES`` is swept against the fp64 oracle by tests/test_gpu_generic_matrix.py,
``SEQUENCES`` (the run-time branches of the kernel) at one field of 256 threads and one of 640, both with a ragged last slot.
tests/test_generic_matrix_coverage.py parses the sources and fails when a constant, a branch or a kernel changes there without
the tables here following, and runs the oracle alone over every case: no slot band may be without signal.
"""
from tests import ms_matrix as MM
from tests import st_matrix as SM

# adm_ms_gen.h, adm_ms_generic.hip (compared with the source by the coverage test)
GEN_E = 16
NT_FLOOR, NT_ROUND, NT_CAP = 256, 64, 1024
LDS_SLACK, LDS_LIMIT = 64, 160 * 1024 - 256
RED_SLOTS = 16
factor = SM.factor                      # plan_create's radix rule: one mirror for both paths


def threads(py, px):
    """ms_generic_threads: at most GEN_E elements per thread, whole waves, at least four of them."""
    n = py * px
    return max(NT_FLOOR, ((n + GEN_E - 1) // GEN_E + NT_ROUND - 1) // NT_ROUND * NT_ROUND)


def lds_bytes(py, px):
    return (py * px + px + py) * 8 + LDS_SLACK


def supported(py, px):
    """ms_generic_supported."""
    return threads(py, px) <= NT_CAP and lds_bytes(py, px) <= LDS_LIMIT


def geometry(Py, Px):
    n, nt = Py * Px, threads(Py, Px)
    ne = -(-n // nt)
    return dict(n=n, nt=nt, waves=nt // 64, ne=ne, last=n - (ne - 1) * nt, lds_bytes=lds_bytes(Py, Px),
                radix_y=factor(Py), radix_x=factor(Px))


def slot_bands(Py, Px):
    """[start, stop) of the natural-order elements of every register slot j: i = tid + j * nt."""
    g = geometry(Py, Px)
    return [(j * g['nt'], min((j + 1) * g['nt'], g['n'])) for j in range(g['ne'])]


WAVE_COUNTS = tuple(range(4, 17))
SLOT_CLASSES = ('n_lt_one_wave', 'n_lt_256', 'n_eq_256', 'ne_16_full_nt256', 'first_nt_gt_256') + tuple('waves_%d' % w for w in WAVE_COUNTS) + (
    'last_slot_ragged', 'last_slot_one_element', 'n_max_full', 'n_max_ragged')
RADIX_CLASSES = ('pow2_only', 'single_radix_2_3_5_7', 'has_9_3_5_7', 'leftover_prime_small', 'leftover_two_primes', 'leftover_prime_repeated',
                 'leftover_prime_large', 'passes_ge_5', 'four_passes_of_8', 'side_1')
ALL_CLASSES = SLOT_CLASSES + tuple('%s_%s' % (c, ax) for ax in 'yx' for c in RADIX_CLASSES)


def radix_classes(radices):
    out = SM.radix_classes(radices)                     # pow2_only, has_9_3_5_7, leftover_prime_small / _large / _repeated, passes_ge_5
    left = [q for q in radices if q not in SM.PREF]
    if len(radices) == 1 and radices[0] in (2, 3, 5, 7):
        out.add('single_radix_2_3_5_7')
    if len(set(left)) >= 2:
        out.add('leftover_two_primes')
    if radices == [8, 8, 8, 8]:
        out.add('four_passes_of_8')
    if not radices:
        out.add('side_1')
    return out


def classes(Py, Px):
    g, out = geometry(Py, Px), set()
    n, nt, ne = g['n'], g['nt'], g['ne']
    if n < 64:
        out.add('n_lt_one_wave')                     # three waves without an element, idle lanes in the fourth
    if n < NT_FLOOR:
        out.add('n_lt_256')
    if n == NT_FLOOR:
        out.add('n_eq_256')
    if n == NT_FLOOR * GEN_E:
        out.add('ne_16_full_nt256')
    if NT_FLOOR * GEN_E < n <= NT_FLOOR * GEN_E + NT_ROUND:
        out.add('first_nt_gt_256')                   # 4096 < n <= 4160: 320 threads, ne = 13
    out.add('waves_%d' % g['waves'])
    if g['last'] < nt and ne > 1:
        out.add('last_slot_ragged')
    if g['last'] == 1 and ne > 1:
        out.add('last_slot_one_element')
    if n == NT_CAP * GEN_E:
        out.add('n_max_full')
    if n == NT_CAP * GEN_E - 1:
        out.add('n_max_ragged')
    for ax, rad in (('y', g['radix_y']), ('x', g['radix_x'])):
        out |= {'%s_%s' % (c, ax) for c in radix_classes(rad)}
    return out


# the fields of the sweep: oracle_case arguments S = 3, B = 5 (one position over each corner of the object and one inside)
_KW = dict(S=3, B=5)
SHAPES = {s: dict(_KW) for s in (
    (2, 3), (3, 2), (5, 7), (7, 5),                  # n < 64; the single-radix sides
    (1, 64), (64, 1),                                # an axis without a pass
    (13, 17),                                        # n = 221 < 256: a leftover prime on each axis
    (16, 16), (16, 17),                              # n = 256: one full slot; 272: a second slot of 16
    (19, 27),                                        # n = 513 = 2 * 256 + 1: a last slot of one element
    (33, 31),                                        # last slot 255 of 256
    (64, 64), (63, 65), (64, 65),                    # ne = 16 at 256 threads, full and ragged; the first field of 320 threads
    (57, 73),                                        # n = 4161 = 13 * 320 + 1: a last slot of one element beyond 256 threads
    (72, 80), (81, 84), (80, 90), (95, 96), (100, 100), (104, 105), (3, 4096), (4096, 3), (112, 117), (113, 120),      # 6 ... 14 waves
    (11, 143), (143, 11),                            # 143 = 11 * 13: two leftover primes on one axis
    (8, 1890), (1890, 8),                            # 2 * 9 * 3 * 5 * 7: five passes; 15 waves
    (8, 2039), (2039, 8),                            # one 2039-term pass; 16 waves
    (105, 143), (143, 105), (121, 121),
    (127, 129), (129, 127),                          # n = 16383: a last slot of 1023
    (128, 128), (8, 2048), (2048, 8),                # n = 16384
)}
for _s in SHAPES:
    if _s[0] == _s[1] and _s[0] in MM.SIZES:
        SHAPES[_s]['generic'] = True                 # 16 x 16, 64 x 64: a tuned kernel exists, the plan is told to take this one
# refused by the LDS bound (Py*Px + Px + Py complex numbers), not by n > 16384; 3 x 4096 is on the accepted side of it
LDS_REFUSED = [(4, 4096), (2, 8192), (1, 16384)]
LDS_ACCEPTED = (3, 4096)

# the fields at which every launch sequence runs: 256 threads and more, each with a ragged last slot
SEQUENCE_SHAPES = {'nt256': (33, 31), 'nt640': (100, 100)}

# the run-time branches of ms_generic_kernel: oracle_case arguments (S = 3, B = 5 unless given); 'forward_only', 'pred_null' and
# 'gprobe_null' are flags of the test (a second launch compared bit for bit), not of oracle_case
_SEQ_DEFAULTS = dict(S=3, B=5)
_DISTS = [1e-4, 2e-4, 3.5e-4]
SEQUENCES = {
    'far_sign_p1': dict(),
    'far_sign_m1': MM.VARIANTS['far_sign_m1'],
    'normalize_fft': dict(normalize_fft=True),
    'normalize_fft_sign_m1_no_cache': MM.VARIANTS['far_ortho_sign_m1'],
    'exit_wave': MM.VARIANTS['near_field'],
    'fresnel': dict(free_prop=1e-4),
    'three_distances_shared_probe': dict(free_prop=_DISTS, B=6),                 # b % n_hfree with one probe set: generic plans only
    'three_distances_shared_probe_modes': dict(free_prop=_DISTS, B=6, n_modes=3),
    'three_distances_pp': dict(free_prop=_DISTS, pp='probes', B=6),
    'S1': dict(S=1),
    'three_modes': dict(n_modes=3),
    'three_modes_fresnel': MM.VARIANTS['fresnel_modes'],
    'three_modes_sign_m1': MM.VARIANTS['far_sign_m1_modes'],
    'real_imag': dict(unknown_type='real_imag'),
    'real_imag_modes': dict(unknown_type='real_imag', n_modes=3),
    'delta_beta_no_cache': dict(transmission_cache=False),
    'binning2_S5': dict(binning=2, S=5),
    'binning3_S7_modes': dict(binning=3, S=7, n_modes=3),
    'poisson_magnitude': dict(MM.VARIANTS['poisson_magnitude'], seed=1),
    'poisson_intensity_modes': dict(MM.VARIANTS['poisson_intensity_modes'], seed=1),
    'beamstop': MM.VARIANTS['beamstop'],
    'beamstop_modes_exit_wave': MM.VARIANTS['beamstop_modes_near'],
    'pp_probes_modes': dict(pp='probes', n_modes=3),
    'forward_only': dict(forward_only=True),
    'forward_only_modes_fresnel': dict(forward_only=True, n_modes=3, free_prop=1e-4),
    'pred_null': dict(pred_null=True, n_modes=3),
    'gprobe_null': dict(gprobe_null=True),
}
SEQUENCE_CASES = [(name, cls) for name in SEQUENCES for cls in SEQUENCE_SHAPES]
_FLAGS = ('forward_only', 'pred_null', 'gprobe_null')


def sequence_kw(name):
    """The oracle_case arguments of a sequence and the set of its test flags."""
    kw = dict(_SEQ_DEFAULTS, **SEQUENCES[name])
    return kw, {f for f in _FLAGS if kw.pop(f, False)}


REQUIRED_FEATURES = ('far_det_inverse_0', 'far_det_inverse_1', 'normalize_fft', 'exit_wave', 'fresnel', 'multi_distance_shared_probe',
                     'multi_distance_shared_probe_modes', 'multi_distance_pp', 'S1', 'S_gt_1', 'one_mode', 'three_modes',
                     'modes_parked_fresnel', 'modes_parked_det_inverse', 'delta_beta_cache', 'delta_beta_no_cache', 'real_imag',
                     'real_imag_modes', 'binning2_partial_last_bin', 'binning3_partial_last_bin', 'poisson_magnitude', 'poisson_intensity',
                     'beamstop', 'pp_probes', 'pp_probes_modes', 'forward_only', 'pred_null', 'gprobe_null')


def features(name):
    """What a sequence exercises of the kernel's run-time branches."""
    kw, flags = sequence_kw(name)
    fp, M = kw.get('free_prop', 'inf'), kw.get('n_modes', 1)
    inverse = kw.get('sign_convention', 1) == -1
    out = {'S1' if kw['S'] == 1 else 'S_gt_1', 'three_modes' if M == 3 else 'one_mode'} | flags
    if isinstance(fp, list):
        out.add('multi_distance_pp' if kw.get('pp') else 'multi_distance_shared_probe_modes' if M > 1 else 'multi_distance_shared_probe')
    elif fp == 'inf':
        out.add('far_det_inverse_%d' % inverse)
        if M > 1 and inverse:
            out.add('modes_parked_det_inverse')
    else:
        out.add('exit_wave' if fp == 0 else 'fresnel')
        if M > 1 and fp != 0:
            out.add('modes_parked_fresnel')
    binning = kw.get('binning', 1)
    if kw.get('unknown_type', 'delta_beta') == 'real_imag':
        out.add('real_imag_modes' if M > 1 else 'real_imag')
    else:
        out.add('delta_beta_cache' if kw.get('transmission_cache', True) and binning == 1 else 'delta_beta_no_cache')
    if binning > 1 and kw['S'] % binning:
        out.add('binning%d_partial_last_bin' % binning)
    if kw.get('loss') == 'poisson':
        out.add('poisson_%s' % kw['raw_data_type'])
    if kw.get('pp') == 'probes':
        out.add('pp_probes_modes' if M > 1 else 'pp_probes')
    out |= {f for f, on in (('beamstop', kw.get('beamstop')), ('normalize_fft', kw.get('normalize_fft'))) if on}
    return out


# the transposed problem: a five-pass and a two-leftover-prime axis exchanged between x and y
TRANSPOSED_PAIRS = [(8, 1890), (11, 143)]

# every __global__ kernel of adm_ms_generic.hip -> (test module, tests) that run it at the geometries above
KERNELS = {
    'ms_generic_kernel': ('test_gpu_generic_matrix', ('test_shapes_vs_oracle', 'test_sequences_vs_oracle', 'test_transposed_problem_agrees',
                                                      'test_two_launches_give_identical_bits_at_the_largest_ragged_field',
                                                      'test_flagged_launches_keep_the_other_outputs_bits')),
}

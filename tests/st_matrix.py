"""The launch geometries of the streamed multislice path (adm_ms_streamed.hip) and the fields that reach each of them (test
infrastructure only).

``geometry`` mirrors the launch arithmetic of ms_streamed_launch (rows per row workgroup) and adm_ms_col.h (st_cw, st_col_threads,
st_col_geom) and factor()
of adm_api.hip; ``classes`` names what a field exercises of it: how the rows fall into row workgroups, which column workgroup
runs, what radix passes its two axes take.  ``SHAPES`` is swept against the fp64 oracle by tests/test_gpu_streamed_matrix.py,
``SEQUENCES`` (the launch-sequence variants of ms_streamed_launch) at one field of each of the column classes beyond 256 threads.
tests/test_streamed_matrix_coverage.py parses the kernel source and fails when a constant, a branch or a kernel changes there
without the tables here following.
"""
from tests import ms_matrix as MM

# adm_ms_streamed.hip, adm_ms_col.h, adm_ms_gen.h, factor() of adm_api.hip (compared with the source by the coverage test)
ST_ROW_NT, ST_ROW_E = 256, 8
ST_ROW_ELEMS = ST_ROW_NT * ST_ROW_E
ST_COL_NT = 512
ST_MAX_SIDE = 2048
ST_MAX_SLICES = 1024
GEN_E = 16
PREF = (8, 4, 2, 9, 3, 5, 7)
MAX_RADICES = 8


def st_cw(py):
    return 8 if py <= ST_COL_NT * GEN_E // 8 else 4


def st_col_threads(py):
    n = py * st_cw(py)
    return max(256, ((n + GEN_E - 1) // GEN_E + 63) // 64 * 64)


def factor(n):
    """The radix list of a side: the preferred radices as often as they divide, then the odd numbers from 11 (the primes left)."""
    r = []
    for q in PREF:
        while n > 1 and n % q == 0 and len(r) < MAX_RADICES:
            r.append(q)
            n //= q
    q = 11
    while n > 1 and len(r) < MAX_RADICES:
        while n % q == 0 and len(r) < MAX_RADICES:
            r.append(q)
            n //= q
        q += 2
    assert n == 1, 'more than %d radices' % MAX_RADICES
    return r


def geometry(Py, Px):
    assert 1 <= Py <= ST_MAX_SIDE and 1 <= Px <= ST_MAX_SIDE, (Py, Px)
    unclipped = max(1, ST_ROW_ELEMS // Px)
    rows = min(unclipped, Py)
    ngr = -(-Py // rows)
    cw, cnt = st_cw(Py), st_col_threads(Py)
    ncg = -(-Px // cw)
    return dict(rows=rows, rows_unclipped=unclipped, n_row_groups=ngr, rows_last=Py - (ngr - 1) * rows,
                row_ne=-(-rows * Px // ST_ROW_NT), row_ne_last=-(-(Py - (ngr - 1) * rows) * Px // ST_ROW_NT),
                cw=cw, col_threads=cnt, n_col_groups=ncg, cw_last=Px - (ncg - 1) * cw,
                col_ne=-(-Py * min(cw, Px) // cnt), col_lds_bytes=(Py * cw + Py) * 8, det_lds_bytes=(Py * cw + Py) * 8 + Py * cw * 4,
                radix_y=factor(Py), radix_x=factor(Px))


def row_bands(Py, Px):
    """[start, stop) of the rows of every row workgroup."""
    g = geometry(Py, Px)
    return [(r0, min(r0 + g['rows'], Py)) for r0 in range(0, Py, g['rows'])]


def col_bands(Py, Px):
    """[start, stop) of the columns of every column workgroup."""
    g = geometry(Py, Px)
    return [(c0, min(c0 + g['cw'], Px)) for c0 in range(0, Px, g['cw'])]


ROW_CLASSES = ('rows_many_even', 'rows_many_ragged', 'rows_clipped_to_Py', 'row_single_ragged', 'row_single_full')
COL_CLASSES = ('cw8_nt256', 'cw8_nt_gt256', 'cw4', 'nt_nonpow2_waves', 'nt512', 'colgroup_ragged', 'field_narrower_than_cw', 'Py_1024',
               'Py_1025')
RADIX_CLASSES = ('pow2_only', 'has_9_3_5_7', 'leftover_prime_small', 'leftover_prime_large', 'leftover_prime_repeated', 'passes_ge_5')
ALL_CLASSES = ROW_CLASSES + COL_CLASSES + tuple('%s_%s' % (c, ax) for ax in 'yx' for c in RADIX_CLASSES)


def radix_classes(radices):
    out = set()
    left = [q for q in radices if q not in PREF]
    if radices and all(q in (8, 4, 2) for q in radices):
        out.add('pow2_only')
    if any(q in (9, 3, 5, 7) for q in radices):
        out.add('has_9_3_5_7')
    if any(11 <= q <= 127 for q in left):
        out.add('leftover_prime_small')
    if any(q > 127 for q in left):
        out.add('leftover_prime_large')
    if len(left) != len(set(left)):
        out.add('leftover_prime_repeated')
    if len(radices) >= 5:
        out.add('passes_ge_5')
    return out


def classes(Py, Px):
    g, out = geometry(Py, Px), set()
    # rows: the row workgroups of st_row_kernel
    if g['rows_unclipped'] > Py:
        out.add('rows_clipped_to_Py')                        # one workgroup of fewer rows than 2048 elements would hold
    elif g['rows'] > 1:
        out.add('rows_many_even' if g['rows_last'] == g['rows'] else 'rows_many_ragged')
    else:
        out.add('row_single_full' if Px == ST_ROW_ELEMS else 'row_single_ragged')     # full: all ST_ROW_E passes of all threads
    # columns: the column workgroups of the five column kernels
    nt = g['col_threads']
    if g['cw'] == 8:
        out.add('cw8_nt256' if nt == 256 else 'cw8_nt_gt256')
    else:
        out.add('cw4')
    waves = nt // 64
    if waves & (waves - 1):
        out.add('nt_nonpow2_waves')
    if nt == ST_COL_NT:
        out.add('nt512')
    if Px < g['cw']:
        out.add('field_narrower_than_cw')
    elif g['cw_last'] < g['cw']:
        out.add('colgroup_ragged')
    if Py in (1024, 1025):
        out.add('Py_%d' % Py)
    for ax, rad in (('y', g['radix_y']), ('x', g['radix_x'])):
        out |= {'%s_%s' % (c, ax) for c in radix_classes(rad)}
    return out


# (Py, Px) -> oracle_case arguments.  B and S are small so that the CPU oracle stays affordable; B >= 4 keeps one position
# hanging over each corner of the object.
SHAPES = {
    (24, 24): dict(S=3, B=5),                    # a tiny field forced onto the path: the row group clipped to Py
    (5, 2048): dict(S=3, B=5),                   # one full row of 2048 per row workgroup
    (2048, 5): dict(S=3, B=5),                   # 512 threads, 4 columns + a last group of 1
    (2048, 3): dict(S=3, B=5),                   # the whole field narrower than cw = 4
    (520, 7): dict(S=3, B=5),                    # ... and than cw = 8, in a workgroup of 320 threads
    (130, 1536): dict(S=3, B=5),                 # one ragged row (6 of 8 elements per thread)
    (640, 136): dict(S=3, B=5),                  # 320 threads
    (768, 264): dict(S=3, B=5, n_modes=2),       # 384 threads
    (896, 130): dict(S=3, B=5),                  # 448 threads, last column group of 2
    (1000, 243): dict(S=3, B=5),                 # 512 threads of which 500 hold elements; 243 = 9 * 9 * 3
    (1024, 1024): dict(S=2, B=4),                # the largest cw = 8 field: the LDS layout at its full size
    (1025, 132): dict(S=3, B=5),                 # the smallest cw = 4 field
    (1031, 24): dict(S=3, B=5),                  # one direct-sum pass of 1031 along y
    (24, 2039): dict(S=3, B=5),                  # one direct-sum pass of 2039 along x
    (257, 521): dict(S=3, B=5),
    (169, 1331): dict(S=3, B=5),                 # 13 * 13, 11 * 11 * 11
    (135, 201): dict(S=3, B=5, n_modes=2),
    (1152, 12): dict(S=3, B=5),
    (1890, 140): dict(S=3, B=5),                 # 2 * 9 * 3 * 5 * 7: five passes along y
    (140, 1890): dict(S=3, B=5),                 # ... and along x
    (1536, 1280): dict(S=2, B=4, n_modes=2),     # one ragged row per workgroup (5 of 8), 384 threads at cw = 4
    (2048, 2048): dict(S=2, B=4),                # the largest field
}

# the fields at which every launch sequence runs, by column class
SEQUENCE_SHAPES = {'cw8_nt_gt256': (640, 136), 'cw4': (1025, 132)}

# the launch-sequence variants of ms_streamed_launch: oracle_case arguments (S = 3, B = 5 unless given); 'forward_only' is a flag
# of the test, not of oracle_case
_SEQ_DEFAULTS = dict(S=3, B=5)
SEQUENCES = {
    'far_sign_p1': dict(),                                                      # det_inverse 0
    'far_sign_m1': MM.VARIANTS['far_sign_m1'],                                  # det_inverse 1
    'far_sign_m1_modes': MM.VARIANTS['far_sign_m1_modes'],
    'exit_wave': MM.VARIANTS['near_field'],
    'fresnel': dict(free_prop=1e-4),
    'fresnel_modes': MM.VARIANTS['fresnel_modes'],
    'S1_far': dict(S=1),                                                        # the four-launch 2-D case
    'S1_far_modes': dict(S=1, n_modes=3),
    'three_modes': dict(n_modes=3),
    'delta_beta_no_cache': dict(transmission_cache=False),
    'real_imag': dict(unknown_type='real_imag'),
    'real_imag_modes_fresnel': dict(unknown_type='real_imag', n_modes=3, free_prop=1e-4),
    'binning_partial_last_bin': dict(binning=2, S=5),
    'beamstop': MM.VARIANTS['beamstop'],
    'beamstop_modes_exit_wave': MM.VARIANTS['beamstop_modes_near'],
    # (seed 1: with seed 0 and five positions a detector pixel of next to no intensity makes the Poisson gradient so
    # ill-conditioned that the oracle's own fp32 run is 1e-3 / 3e-4 away from its fp64 run at the two fields -- beyond the
    # GENERIC cap of 2e-4 before any kernel has run; the sweep asserts that no case is like that)
    'poisson_magnitude': dict(MM.VARIANTS['poisson_magnitude'], seed=1),
    'poisson_intensity_modes': dict(MM.VARIANTS['poisson_intensity_modes'], seed=1),
    'normalize_fft_modes': MM.VARIANTS['far_ortho_modes'],
    'forward_only': dict(forward_only=True),
    'forward_only_modes_exit_wave': dict(forward_only=True, n_modes=3, free_prop=0),
}
SEQUENCE_CASES = [(name, cls) for name in SEQUENCES for cls in SEQUENCE_SHAPES]


def sequence_kw(name):
    """The oracle_case arguments of a sequence and its forward_only flag."""
    kw = dict(_SEQ_DEFAULTS, **SEQUENCES[name])
    return kw, kw.pop('forward_only', False)


REQUIRED_FEATURES = ('far_det_inverse_0', 'far_det_inverse_1', 'exit_wave', 'fresnel', 'S1', 'S_gt_1', 'one_mode', 'three_modes',
                     'delta_beta_cache', 'delta_beta_no_cache', 'real_imag', 'binning_partial_last_bin', 'beamstop', 'poisson',
                     'normalize_fft', 'forward_only')


def features(name):
    """What a sequence exercises of ms_streamed_launch and of the kernels' run-time branches."""
    kw, fwd = sequence_kw(name)
    fp = kw.get('free_prop', 'inf')
    out = {'S1' if kw['S'] == 1 else 'S_gt_1', 'three_modes' if kw.get('n_modes', 1) == 3 else 'one_mode'}
    if fp == 'inf':
        out.add('far_det_inverse_%d' % (kw.get('sign_convention', 1) == -1))
    else:
        out.add('exit_wave' if fp == 0 else 'fresnel')
    binning = kw.get('binning', 1)
    if kw.get('unknown_type', 'delta_beta') == 'real_imag':
        out.add('real_imag')
    else:
        out.add('delta_beta_cache' if kw.get('transmission_cache', True) and binning == 1 else 'delta_beta_no_cache')
    if binning > 1 and kw['S'] % binning:
        out.add('binning_partial_last_bin')
    out |= {f for f, on in (('beamstop', kw.get('beamstop')), ('poisson', kw.get('loss') == 'poisson'),
                            ('normalize_fft', kw.get('normalize_fft')), ('forward_only', fwd)) if on}
    return out


# sparse multislice and dL/dz at the new geometries: make_case arguments of tests/test_gpu_sparse_multislice.py
SPARSE_CASES = {
    'P640x136_S3': dict(P=(640, 136), S=3, B=5),
    'P1152x12_S4_modes': dict(P=(1152, 12), S=4, M=2, B=5),
    'P1031x24_S3': dict(P=(1031, 24), S=3, B=5),
    'P135x201_S3_real_imag': dict(P=(135, 201), S=3, unknown_type='real_imag'),
    'P2048x5_S3_exit_wave': dict(P=(2048, 5), S=3, free_prop=0, B=5),
    'P1536x1280_S3_B4': dict(P=(1536, 1280), S=3, B=4),
    'P24_S40': dict(P=24, S=40, B=5),            # 39 gaps in st_dd_reduce_kernel
}
# the restatement's own fp32 dL/dz error on these cases (CPU; the sweep asserts >= 1e-6): 2.6e-5, 2.0e-5, 6.5e-5, 7.3e-5, 2.7e-6,
# 7.9e-5, 2.5e-5.  An exit-wave detector averages the rounding errors out: (2048, 5) with B = 11 has 8e-8 and would measure the
# rounding of the fp32 output, not the kernels.

# every __global__ kernel of adm_ms_streamed.hip -> (test module, tests) that run it at the geometries above
_M, _S = 'test_gpu_streamed_matrix', 'test_gpu_sparse_multislice'
KERNELS = {
    'st_row_kernel': (_M, ('test_shapes_vs_oracle', 'test_sequences_vs_oracle')),
    'st_col_conv_kernel<false>': (_M, ('test_shapes_vs_oracle', 'test_sequences_vs_oracle')),
    'st_col_conv_kernel<true>': (_M, ('test_shapes_vs_oracle', 'test_sequences_vs_oracle')),
    'st_det_kernel': (_M, ('test_shapes_vs_oracle', 'test_sequences_vs_oracle')),
    'st_loss_reduce_kernel': (_M, ('test_shapes_vs_oracle', 'test_sequences_vs_oracle')),
    'st_fresnel_table_kernel': (_M, ('test_sparse_vs_restatement',)),
    'st_col_conv_sparse_kernel<false>': (_M, ('test_sparse_vs_restatement',)),
    'st_col_conv_sparse_kernel<true>': (_M, ('test_sparse_vs_restatement',)),
    'st_dd_reduce_kernel': (_M, ('test_sparse_vs_restatement',)),
    'st_sparse_anchor_kernel': (_M, ('test_most_slice_positions',)),
    'st_shift_reduce_kernel': ('test_gpu_prj_offset', ('test_kernels_vs_reference', 'test_geometries_vs_restatement')),
}

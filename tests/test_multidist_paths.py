"""MultiDistModel's host logic that needs no GPU: which of its four forward paths the constructor picks from what the caller
brought, and what _check refuses, by type and full message, with stand-ins for the engines that carry only the attributes the
checks read.  CPU."""
import itertools
from types import SimpleNamespace as NS

import numpy as np
import pytest

from adorym_amd.forward_model import MultiDistModel


def fan_engine(**over):
    return NS(**dict(dict(detector_fanout=True, refine_distances=False, n_dists=3, probe_size=(16, 16), n_det=256), **over))


def ctf_engine(**over):
    return NS(**dict(dict(n_dists=3, ny=16, nx=16, refine_distances=False, raw_data_type='magnitude'), **over))


def registration(**over):
    return NS(**dict(dict(n_dists=3, ny=16, nx=16, raw_data_type='magnitude'), **over))


def projector(obj_size=(16, 16, 8)):
    return NS(obj_size=obj_size)


def model(kind, over, **kw):
    """The model a driver would build for ``kind``, with ``over`` laid over its common_vars_dict."""
    cv = dict(engine=None, holo_engine=NS(n_dists=3), forward_algorithm='fresnel', two_d_mode=True)
    if kind == 'tiles':
        cv.update(tile_engine=NS(), safe_zone_width=2)
    elif kind == 'fanout':
        cv.update(engine=fan_engine(), two_d_mode=False)
    elif kind == 'ctf':
        cv.update(forward_algorithm='ctf', ctf_engine=ctf_engine())
    elif kind == 'ctf3d':
        cv.update(forward_algorithm='ctf', ctf_engine=ctf_engine(), two_d_mode=False, ctf_projector=projector())
    cv.update(over)
    return MultiDistModel(device=None, common_vars_dict=cv, **kw)


# ------------------------------------------------------------------------------------------------------------ (a) path selection
def test_a_bare_model_constructs():
    fm = MultiDistModel()
    assert type(fm._path).__name__ == '_FieldPath'
    assert fm.tile_engine is None and fm.engine is None and not fm.register_3d
    assert fm.argument_ls[10:14] == ['free_prop_cm', 'safe_zone_width', 'prj_affine_ls', 'ctf_lg_kappa'] and len(fm.argument_ls) == 15


@pytest.mark.parametrize('algo,fanout,tiles,proj', list(itertools.product(('fresnel', 'ctf'), (False, True), (False, True), (False, True))))
def test_path_selection(algo, fanout, tiles, proj):
    """CTF first, then the fan-out engine, then the tile engine, then the undivided field: today's rule in today's order."""
    fm = model('field', dict(forward_algorithm=algo, engine=fan_engine() if fanout else None, tile_engine=NS() if tiles else None,
                             ctf_engine=ctf_engine(), ctf_projector=projector() if proj else None,
                             hologram_registration=registration()))
    want = '_CTFPath' if algo == 'ctf' else '_FanoutPath' if fanout else '_TiledPath' if tiles else '_FieldPath'
    assert type(fm._path).__name__ == want
    assert type(fm) is MultiDistModel
    assert fm.register_3d == (want == '_FanoutPath')
    assert (fm.tile_engine is not None) == tiles


def test_constructor_refusals():
    with pytest.raises(ValueError) as e:
        model('field', dict(forward_algorithm='ctf'))
    assert str(e.value) == "MultiDistModel with forward_algorithm='ctf' needs common_vars_dict['ctf_engine'] (an adorym_amd.CTFEngine)"
    with pytest.raises(NotImplementedError) as e:
        model('ctf', {}, loss_function_type='poisson')
    assert str(e.value) == 'MultiDistModel: only the LSQ loss is on the accelerated path'


# ------------------------------------------------------------------------------------------------------------ (b) the refusal table
P3 = 'multi-distance holography of a 3-D object with %s is outside the accelerated path'
PC = "forward_algorithm='ctf' with %s is outside the accelerated path"
PT = '%s with multi-distance data divided into sub-tiles is outside the accelerated path'
TILES = 'data divided into sub-tiles or safe_zone_width > 0'
REG = 'MultiDistModel: hologram_registration was built for another field, number of distances or raw_data_type'
NEEDS_FANOUT = ("MultiDistModel with two_d_mode=False needs common_vars_dict['engine'] built with detector_fanout=True "
                "(an adorym_amd.MultisliceEngine for the sequence of distances)")
SHIFTS = np.zeros((3, 2))
KAPPA = np.array([1.7])
NIE, VE = NotImplementedError, ValueError

# (kind, what is laid over common_vars_dict, _check's arguments (safe_zone_width, ctf_lg_kappa, probe_pos_correction),
#  the exception's type or None for "passes", its full message)
TABLE = [
    # what every path serves
    ('field', {}, (0, None, None), None, None),
    ('field', dict(optimize_free_prop=True, optimize_prj_affine=True, optimize_probe=True), (None, None, None), None, None),
    ('field', dict(optimize_all_probe_pos=True), (0, None, SHIFTS), None, None),
    ('tiles', {}, (2, None, None), None, None),
    ('fanout', {}, (0, None, None), None, None),
    ('ctf', {}, (0, KAPPA, None), None, None),
    ('ctf3d', {}, (0, KAPPA, None), None, None),
    # the three flags that no path serves, in front of everything else
    ('field', dict(optimize_probe_defocusing=True), (0, None, None), NIE, 'optimize_probe_defocusing with MultiDistModel is outside the accelerated path'),
    ('fanout', dict(optimize_probe_pos_offset=True), (0, None, None), NIE, 'optimize_probe_pos_offset with MultiDistModel is outside the accelerated path'),
    ('ctf', dict(optimize_prj_pos_offset=True, unknown_type='real_imag'), (0, KAPPA, None), NIE,
     'optimize_prj_pos_offset with MultiDistModel is outside the accelerated path'),
    ('tiles', dict(optimize_probe_defocusing=True, optimize_prj_pos_offset=True), (2, None, None), NIE,
     'optimize_probe_defocusing with MultiDistModel is outside the accelerated path'),
    # the Fresnel paths
    ('field', dict(optimize_ctf_lg_kappa=True), (0, KAPPA, None), NIE,
     "optimize_ctf_lg_kappa with forward_algorithm='fresnel' is outside the accelerated path"),
    ('fanout', dict(optimize_ctf_lg_kappa=True), (0, KAPPA, None), NIE,
     "optimize_ctf_lg_kappa with forward_algorithm='fresnel' is outside the accelerated path"),
    ('field', dict(optimize_all_probe_pos=True, optimize_prj_affine=True), (0, None, SHIFTS), NIE,
     'optimize_all_probe_pos together with optimize_prj_affine is outside the accelerated path'),
    ('tiles', dict(optimize_all_probe_pos=True), (2, None, SHIFTS), NIE,
     'optimize_all_probe_pos with multi-distance data divided into sub-tiles is outside the accelerated path'),
    ('field', dict(optimize_all_probe_pos=True), (0, None, None), VE, 'optimize_all_probe_pos needs probe_pos_correction [n_dists, 2]'),
    ('fanout', dict(optimize_all_probe_pos=True), (0, None, None), VE, 'optimize_all_probe_pos needs probe_pos_correction [n_dists, 2]'),
    ('tiles', {}, (3, None, None), VE, 'safe_zone_width differs from the width the tile engine was built for'),
    ('tiles', {}, (None, None, None), VE, 'safe_zone_width differs from the width the tile engine was built for'),
    ('tiles', dict(optimize_free_prop=True), (2, None, None), NIE, PT % 'optimize_free_prop'),
    ('tiles', dict(optimize_prj_affine=True), (2, None, None), NIE, PT % 'optimize_prj_affine'),
    ('field', {}, (2, None, None), NIE, 'safe_zone_width > 0 needs the tile engine (the driver builds it)'),
    ('field', dict(two_d_mode=False), (0, None, None), VE, NEEDS_FANOUT),
    ('tiles', dict(two_d_mode=False), (2, None, None), NIE, P3 % TILES),
    ('fanout', dict(two_d_mode=True), (0, None, None), VE,
     'MultiDistModel in two_d_mode takes a HolographyEngine (holo_engine), not an engine with detector_fanout'),
    # a 3-D object: REFUSED_3D_FLAGS, unserved and served
    ('fanout', dict(optimize_free_prop=True), (0, None, None), NIE, P3 % 'optimize_free_prop'),
    ('fanout', dict(optimize_prj_affine=True), (0, None, None), NIE, P3 % 'optimize_prj_affine'),
    ('fanout', dict(optimize_all_probe_pos=True), (0, None, SHIFTS), NIE, P3 % 'optimize_all_probe_pos'),
    ('fanout', dict(rotate_out_of_loop=True), (0, None, None), NIE, P3 % 'rotate_out_of_loop'),
    ('fanout', dict(optimize_free_prop=True, engine=fan_engine(refine_distances=True)), (0, None, None), None, None),
    ('fanout', dict(optimize_prj_affine=True, hologram_registration=registration()), (0, None, None), None, None),
    ('fanout', dict(optimize_free_prop=True, optimize_prj_affine=True, hologram_registration=registration()), (0, None, None), NIE,
     P3 % 'optimize_free_prop'),
    ('fanout', dict(optimize_free_prop=True, optimize_prj_affine=True, engine=fan_engine(refine_distances=True)), (0, None, None), NIE,
     P3 % 'optimize_prj_affine'),
    ('fanout', dict(optimize_free_prop=True, optimize_prj_affine=True, rotate_out_of_loop=True, engine=fan_engine(refine_distances=True),
                    hologram_registration=registration()), (0, None, None), NIE, P3 % 'rotate_out_of_loop'),
    ('fanout', dict(unknown_type='real_imag', optimize_free_prop=True), (0, None, None), NIE, P3 % "unknown_type='real_imag'"),
    ('fanout', dict(tile_engine=NS(), unknown_type='real_imag'), (0, None, None), NIE, P3 % TILES),
    ('fanout', {}, (2, None, None), NIE, P3 % TILES),
    ('fanout', dict(safe_zone_width=2), (0, None, None), NIE, P3 % TILES),
    ('fanout', dict(optimize_prj_affine=True, hologram_registration=registration(n_dists=4)), (0, None, None), VE, REG),
    ('fanout', dict(optimize_prj_affine=True, hologram_registration=registration(ny=32)), (0, None, None), VE, REG),
    ('fanout', dict(optimize_prj_affine=True, hologram_registration=registration(raw_data_type='intensity')), (0, None, None), VE, REG),
    ('fanout', dict(hologram_registration=registration(n_dists=4)), (0, None, None), None, None),
    ('fanout', dict(optimize_prj_affine=True, hologram_registration=registration(), engine=fan_engine(n_det=200)), (0, None, None), NIE,
     'multi-distance holography of a 3-D object with optimize_prj_affine and a beamstop is outside the accelerated path'),
    # the CTF model: CTF_REFUSED_FLAGS, unserved and served
    ('ctf', dict(optimize_probe=True), (0, KAPPA, None), NIE, PC % 'optimize_probe'),
    ('ctf', dict(optimize_free_prop=True), (0, KAPPA, None), NIE, PC % 'optimize_free_prop'),
    ('ctf', dict(optimize_prj_affine=True), (0, KAPPA, None), NIE, PC % 'optimize_prj_affine'),
    ('ctf', dict(optimize_all_probe_pos=True), (0, KAPPA, None), NIE, PC % 'optimize_all_probe_pos'),
    ('ctf', dict(optimize_free_prop=True, ctf_engine=ctf_engine(refine_distances=True)), (0, KAPPA, None), None, None),
    ('ctf', dict(optimize_prj_affine=True, hologram_registration=registration()), (0, KAPPA, None), None, None),
    ('ctf3d', dict(optimize_free_prop=True, optimize_prj_affine=True, ctf_engine=ctf_engine(refine_distances=True),
                   hologram_registration=registration()), (0, KAPPA, None), None, None),
    ('ctf', dict(optimize_free_prop=True, optimize_prj_affine=True, hologram_registration=registration()), (0, KAPPA, None), NIE,
     PC % 'optimize_free_prop'),
    ('ctf', dict(optimize_probe=True, optimize_free_prop=True, ctf_engine=ctf_engine(refine_distances=True)), (0, KAPPA, None), NIE,
     PC % 'optimize_probe'),
    ('ctf', dict(optimize_ctf_lg_kappa=True), (0, KAPPA, None), None, None),
    ('ctf', dict(unknown_type='real_imag', n_probe_modes=3), (0, KAPPA, None), NIE, PC % "unknown_type='real_imag'"),
    ('ctf', dict(n_probe_modes=3, optimize_probe=True), (0, KAPPA, None), NIE, PC % 'n_probe_modes != 1'),
    ('ctf', dict(two_d_mode=False), (0, KAPPA, None), NIE, PC % 'two_d_mode=False'),
    ('ctf', dict(tile_engine=NS()), (0, KAPPA, None), NIE, PC % TILES),
    ('ctf', {}, (3, KAPPA, None), NIE, PC % TILES),
    ('ctf3d', dict(safe_zone_width=3), (0, KAPPA, None), NIE, PC % TILES),
    ('ctf', {}, (0, None, None), VE, "forward_algorithm='ctf' needs ctf_lg_kappa"),
    ('ctf', dict(optimize_prj_affine=True, hologram_registration=registration(n_dists=2)), (0, KAPPA, None), VE, REG),
    ('ctf', dict(optimize_prj_affine=True, hologram_registration=registration(nx=32)), (0, KAPPA, None), VE, REG),
    ('ctf', dict(optimize_prj_affine=True, hologram_registration=registration(raw_data_type='intensity')), (0, KAPPA, None), VE, REG),
    ('ctf', dict(optimize_prj_affine=True, hologram_registration=registration(), ctf_engine=ctf_engine(raw_data_type='intensity')),
     (0, KAPPA, None), VE, "MultiDistModel: forward_algorithm='ctf' with optimize_prj_affine needs a ctf_engine built with "
                           "raw_data_type='magnitude' (the registered holograms are magnitudes already)"),
    # ... of a 3-D object
    ('ctf3d', dict(rotate_out_of_loop=True), (0, KAPPA, None), NIE, PC % 'two_d_mode=False and rotate_out_of_loop'),
    ('ctf3d', dict(n_ranks=2), (0, KAPPA, None), NIE, PC % 'two_d_mode=False and more than one rank'),
    ('ctf3d', dict(ctf_engine=ctf_engine(ny=24), ctf_projector=projector((24, 16, 8))), (0, KAPPA, None), NIE,
     PC % 'two_d_mode=False and a field of 24 x 16 on a 24 x 16 x 8 object (sides: powers of two in [16, 2048])'),
    ('ctf3d', dict(ctf_engine=ctf_engine(nx=8), ctf_projector=projector((16, 8, 8))), (0, KAPPA, None), NIE,
     PC % 'two_d_mode=False and a field of 16 x 8 on a 16 x 8 x 8 object (sides: powers of two in [16, 2048])'),
    ('ctf3d', dict(ctf_engine=ctf_engine(ny=4096), ctf_projector=projector((4096, 16, 8))), (0, KAPPA, None), NIE,
     PC % 'two_d_mode=False and a field of 4096 x 16 on a 4096 x 16 x 8 object (sides: powers of two in [16, 2048])'),
    ('ctf3d', dict(ctf_projector=projector((16, 32, 4))), (0, KAPPA, None), NIE,
     PC % 'two_d_mode=False and a field of 16 x 16 on a 16 x 32 x 4 object (sides: powers of two in [16, 2048])'),
]


@pytest.mark.parametrize('row', range(len(TABLE)))
def test_refusal_table(row):
    kind, over, args, exc, message = TABLE[row]
    fm = model(kind, over)
    if exc is None:
        assert fm._check(*args) is None
        return
    with pytest.raises(exc) as e:
        fm._check(*args)
    assert type(e.value) is exc and str(e.value) == message


def test_the_table_covers_every_refused_flag():
    named = {k for _, over, _, exc, _ in TABLE if exc is not None for k in over}
    assert set(MultiDistModel.REFUSED_3D_FLAGS) | set(MultiDistModel.CTF_REFUSED_FLAGS) <= named

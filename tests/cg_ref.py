"""NumPy restatement of the conjugate-gradient object optimiser: CGOptimizer.apply_gradient (adorym/optimizers.py:594-704) with the
backtracking search of adorym/linesearch.py (a new search object per update, so both of the reference's classes start from
step_size / |s| and behave alike), inside the control flow of the reference driver for one rank and update_scheme='immediate'.
Loss and gradient come from oracle.adorym_oracle.  tests/test_cg_ref_vs_golden.py holds it to the reference's own fp64 runs (golden
F33); the GPU tests hold adorym_amd to it."""
import numpy as np

from oracle import adorym_oracle as O

SUFF_DECR, CONTRACTION, THRESHOLD = 1e-4, 0.5, 1e-10
MACHINE_MAXITER = int(np.ceil(np.log(np.finfo(np.float32).eps) / np.log(CONTRACTION)))        # 23


def line_search(trial, f0, df0, norm, step_size, max_backtracking_iter=None, normalize_alpha=True):
    """trial(alpha) -> loss.  Returns (accepted alpha or 0., step_count, [(alpha, loss), ...])."""
    maxiter = MACHINE_MAXITER if max_backtracking_iter is None else min(int(max_backtracking_iter), MACHINE_MAXITER)
    alpha = step_size / norm if normalize_alpha else step_size
    f = trial(alpha)
    trials = [(float(alpha), float(f))]
    while f > f0 + SUFF_DECR * alpha * df0 and len(trials) <= maxiter and alpha > THRESHOLD:
        alpha = CONTRACTION * alpha
        f = trial(alpha)
        trials.append((float(alpha), float(f)))
    return (float(alpha) if f <= f0 else 0.), len(trials), trials


def cg_update(x, g, d_old, s, i_batch, loss_at, f0, step_size=1., max_backtracking_iter=None, normalize_alpha=True, **unused):
    """One update.  x, g, d_old, s: arrays of one dtype; loss_at(x_trial) -> float.  Returns (x_new, d_old_new, s_new, record);
    x_new is x itself when the search fails.  beta = 0 when sum d_old^2 = 0 (the reference divides)."""
    d = -g
    raw = 0.
    if i_batch > 0:
        b = float(np.sum(d_old * d_old))
        raw = float(np.sum(d * (d - d_old))) / b if b > 0 else 0.
    beta = max(raw, 0.)
    s_new = d + x.dtype.type(beta) * s
    check = float(np.sum(s_new * g))
    if check >= 0:
        s_new = d
    df0 = float(np.sum(s_new * g))
    norm = float(np.sqrt(np.sum(s_new * s_new)))
    alpha, count, trials = line_search(lambda a: float(loss_at(x + x.dtype.type(a) * s_new)), f0, df0, norm, step_size,
                                       max_backtracking_iter, normalize_alpha)
    x_new = x + x.dtype.type(alpha) * s_new if alpha != 0 else x
    rec = dict(i_batch=int(i_batch), beta_raw=raw, beta=beta, descent_check=check, f0=float(f0), df0=df0, norm=norm, trials=trials,
               alpha=alpha, step_count=count, last_loss=trials[-1][1])
    return x_new, d, s_new, rec


def reconstruct_cg(prj, obj_init, probe, probe_pos, theta_ls, phys, n_epochs=1, minibatch_size=1, options=None, non_negativity=False,
                   two_d_mode=False, dtype='float64', optimizer_batch_number_increment='angle', on_update=None):
    """The driver's loop (ptychography.py:783-1295; oracle.reconstruct's, for CG).  ``options``: the optimiser's options_dict.
    ``on_update(dict)`` sees the state every update starts from: x, g, d_old, s, i_batch, i_theta, ind, f0.
    Returns (object, logged losses, per-update records, first gradient).  The logged loss of a minibatch is the loss of the LAST
    TRIAL of its search: current_loss as the search leaves it (ptychography.py:1251)."""
    dt = np.dtype(dtype)
    x = np.stack([obj_init[0], obj_init[1]], -1).astype(dt)
    if non_negativity:
        x[x < 0] = 0            # initialize_object_for_dp clips the guess (adorym/util.py:71-125)
    d_old, s = np.zeros_like(x), np.zeros_like(x)
    pc = np.asarray(probe)
    pos_int = np.round(np.asarray(probe_pos)).astype(int)
    tables, losses, records, first_grad = {}, [], [], None
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, len(theta_ls), len(probe_pos), minibatch_size, 1, 'immediate', two_d_mode=two_d_mode)
        i_opt = 0
        for i_batch in range(len(batches)):
            i_theta, ind = O.rank_batch(batches, i_batch, 0, minibatch_size, 1)
            coords = None
            if not two_d_mode:
                if i_theta not in tables:
                    tables[i_theta] = O.rotation_coords(x.shape[:3], theta_ls[i_theta], dt)
                coords = tables[i_theta]
            pos, meas = pos_int[ind], np.abs(prj[i_theta, ind])
            f0, _, g, _ = O.forward_adjoint_object(x, coords, pc, pos, meas, phys, dt)
            g = g.astype(dt)
            if first_grad is None:
                first_grad = g.copy()
            if on_update is not None:
                on_update(dict(x=x, g=g, d_old=d_old, s=s, i_batch=i_opt, i_theta=i_theta, ind=ind, f0=float(f0)))
            loss_at = lambda xt: O.forward_adjoint_object(xt, coords, pc, pos, meas, phys, dt)[0]
            x, d_old, s, rec = cg_update(x, g, d_old, s, i_opt, loss_at, float(f0), **(options or {}))
            x = O.apply_constraints(x, non_negativity, 'normal', None)
            records.append(rec)
            losses.append(rec['last_loss'])
            last_of_theta = i_batch == len(batches) - 1 or int(batches[i_batch + 1][0, 0]) != int(batches[i_batch][0, 0])
            if optimizer_batch_number_increment != 'angle' or last_of_theta:
                i_opt += 1
    return x, losses, records, first_grad


def golden_run(g, name, inp, E, runs, two_d_inputs, prj3d, dtype='float64', on_update=None):
    """Run fixture ``name`` of golden F33 (``g``: the loaded file; ``runs``, ``two_d_inputs``: tests/cg_matrix.py) -> reconstruct_cg's result."""
    spec = runs[name]
    N, P = E['N'], E['P']
    phys = O.Physics((P, P), E['energy_ev'], E['psize_cm'], free_prop_cm='inf')
    probe = inp['probe_mag'] * np.exp(1j * inp['probe_phase'])
    options = dict(spec.get('options') or {}, step_size=float(g[name + '_learning_rate']))
    if spec['three_d']:
        prj, guess, theta_ls = prj3d, inp['guess'], inp['theta_ls']
    else:
        prj, guess, theta_ls = g[name + '_prj'].astype(np.float64), two_d_inputs(inp, N)[1], inp['theta_ls'][:1]
    return reconstruct_cg(prj, guess, probe, inp['probe_pos'], theta_ls, phys, n_epochs=spec['n_epochs'], minibatch_size=spec['minibatch_size'],
                          options=options, non_negativity=bool(spec.get('non_negativity')), two_d_mode=not spec['three_d'], dtype=dtype,
                          on_update=on_update)

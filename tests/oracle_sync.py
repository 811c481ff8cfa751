"""Copying the CPU oracle's solver state into a GPU handle (TEST INFRASTRUCTURE), shared by the GPU test modules that run a stage
kernel and the oracle's function on identical inputs."""
import numpy as np

SYNC = ["nominal_states", "nominal_actions", "states", "actions", "jacobian_state", "jacobian_action",
        "gradient_state", "gradient_action", "hessian_state_state", "hessian_action_action", "hessian_action_state",
        "K", "k", "violations", "constraint_dual", "constraint_penalty", "active_set"]


def sync_from_oracle(sol, refs, T):
    """Copy the oracle's state into the GPU handle so that a stage starts from identical inputs."""
    n, m, B = sol.nx, sol.nu, sol.B
    for name in SYNC:
        sol.set_buffer(name, np.stack([r.buffer(name) for r in refs]))
    g = [r.buffer("gradient") for r in refs]
    sol.set_buffer("gradient_state_lagrangian", np.stack([v[:(T - 1) * n] for v in g]))
    sol.set_buffer("gradient_action_lagrangian", np.stack([v[T * n:] for v in g]))
    sc = sol.buffer("_scalars")
    for b, r in enumerate(refs):
        st = r.stats()
        sc[b, 0], sc[b, 1], sc[b, 2], sc[b, 3] = st.objective, st.max_violation, st.step_size, st.status
        sc[b, 9] = 0.0      # states_eq_nominal shortcut off: always evaluate both trajectories
    sol.set_buffer("_scalars", sc)

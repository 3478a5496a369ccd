"""Cases for the BC policy forward at network_dim = 128: the four cases.  The seeded state dict, the eager float32 stand-in
(the yardstick's float32 side), the inputs, masks, the yardstick and the rule's host program are tests/bc_cases.py's own, the
float64 restatement tests/bc_reference.py's: each takes the width as an argument or from the state dict."""
from gpudrive_lab_amd import bc_policy as BP
from tests import bc_cases as BC
from tests import bc_reference as REF

DIM = 128

# name -> (B, A, R, cfg).  wide_min: samples a, b, c (every partner masked, every road masked, one key left), L = 264, 63 and 200
# keys (no multiples of 32), odd first-layer kin (6 and 13).  wide_sweep: the reference sweep's model itself.  wide_a128: 127 keys,
# L = 328, branch > fusion (the rg_attn layers sit past ro_attn's in the blob), sample d (the zero-prefix window).  wide_chunks:
# more rows than a small chunk, for chunk_rows 2 against 8.
CASES = {
    "wide_min": (3, 64, 1, BC._cfg((1, 1), 0, 1, -20.0)),
    "wide_sweep": (3, 64, 5, BC._cfg((4, 3), 2, 6, -20.0)),
    "wide_a128": (2, 128, 2, BC._cfg((1, 2), 1, 2, -20.0)),
    "wide_chunks": (5, 64, 1, BC._cfg((1, 1), 0, 6, -20.0)),
}
GOLDEN_CASES = ("wide_min", "wide_sweep", "wide_a128")


def shapes(R, cfg, network_dim=DIM):
    return BP.expected_shapes(R, cfg["num_layer"], cfg["head_num_layers"], cfg["n_components"], network_dim=network_dim)


_CASE = {}


def case(name):
    """Everything a test needs of one case, computed once and shared (leave it unchanged): the state dict, the inputs, the
    float64 restatement with its nll, the float32 stand-in and the yardstick E per output."""
    if name not in _CASE:
        B, A, R, cfg = CASES[name]
        sd = BC.state_dict(R, cfg, network_dim=DIM)
        obs, pm, rm, expert, u, z, kinds = BC.inputs(B, A, R)
        ref = REF.forward(sd, obs, pm, rm, A, **cfg)
        ref["nll"] = REF.nll(ref["means"], ref["log_covariances"], ref["weights"], expert[:, 0])
        f32 = BC.standin_float32(sd, obs, pm, rm, A, cfg, expert)
        _CASE[name] = dict(B=B, A=A, R=R, cfg=cfg, sd=sd, obs=obs, pm=pm, rm=rm, expert=expert, u=u, z=z, kinds=kinds, ref=ref,
                           f32=f32, E=BC.yardstick(f32, ref))
    return _CASE[name]

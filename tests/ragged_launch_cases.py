"""The launch lists tests/test_ragged_launch_order_gpu.py compares against: for each of its cases, the names of the library
entries (every launch goes through _lib.call) of the second call on one attacker and victim, in order.

They were recorded with that file's own record() on the parent commit f2c74fe ("GeoA3 device loop: clouds of different sizes
in one batch"), before the ragged host code moved into ragged.py — not on the tree that carries this file: the test asks
whether the move changed a launch, so its expectation must not come from the moved code. A change that alters a list on
purpose records it again on ITS parent and says so here.

Every name is written without its "pc3d_" prefix and "_f32" suffix."""


def _names(text):
    return ["pc3d_" + w + "_f32" for w in text.split()]


EXPECTED = {
    "cw_dense": _names("""
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear_nn
        linear pointmlp3_max_fwd linear linear cls_tail linear_book linear pointmlp3_max_bwd linear_pre linear
        pointmlp3_max_bwd_update pointmlp3_max_fwd linear_nn linear pointmlp3_max_fwd linear linear cls_tail
        linear_book linear pointmlp3_max_bwd linear_pre linear pointmlp3_max_bwd_update pointmlp3_max_fwd linear
        linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear linear
    """),
    "cw_ragged": _names("""
        pad_ragged pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pad_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn cw_update_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn cw_update_ragged pointmlp3_max_fwd
        linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear linear
    """),
    "cw_ragged_single_point": _names("""
        pad_ragged pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pad_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn cw_update_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn cw_update_ragged pointmlp3_max_fwd
        linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear linear
    """),
    "knn_dense": _names("""
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear pointmlp3_max_fwd linear linear cls_tail linear linear pointmlp3_max_bwd linear_pre linear
        pointmlp3_max_bwd knn_hint nn knn_attack_update pointmlp3_max_fwd linear linear pointmlp3_max_fwd linear
        linear cls_tail linear linear pointmlp3_max_bwd linear_pre linear pointmlp3_max_bwd knn_hint nn
        knn_attack_update pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear linear pointmlp3_max_fwd linear linear linear
    """),
    "knn_ragged": _names("""
        pad_ragged pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pad_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged knn_ragged nn knn_attack_update_ragged
        pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear cls_tail linear linear
        pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged knn_ragged nn knn_attack_update_ragged
        pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear
        linear linear pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
        pointmlp3_max_fwd linear linear linear
    """),
    "geoa3_dense": _names("""
        knn_hint estimate_normal knn_hint kappa pointmlp3_max_fwd linear linear pointmlp3_max_fwd linear linear
        linear cls_loss linear linear linear pointmlp3_max_bwd linear_pre linear pointmlp3_max_bwd nn nn knn_hint
        geoa3_update pointmlp3_max_fwd linear linear pointmlp3_max_fwd linear linear linear cls_loss linear linear
        linear pointmlp3_max_bwd linear_pre linear pointmlp3_max_bwd nn nn knn_hint geoa3_update pointmlp3_max_fwd
        linear linear linear pointmlp3_max_fwd linear linear linear
    """),
    "geoa3_ragged": _names("""
        pad_ragged pad_ragged knn_ragged estimate_normal pad_ragged pad_ragged pad_ragged knn_ragged kappa
        pad_ragged pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear linear cls_loss
        linear linear linear pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn nn knn_ragged
        geoa3_update_ragged pointmlp3_max_fwd_ragged linear linear pointmlp3_max_fwd_ragged linear linear linear
        cls_loss linear linear linear pointmlp3_max_bwd_ragged linear_pre linear pointmlp3_max_bwd_ragged nn nn
        knn_ragged geoa3_update_ragged pointmlp3_max_fwd linear linear linear pointmlp3_max_fwd linear linear linear
    """),
}

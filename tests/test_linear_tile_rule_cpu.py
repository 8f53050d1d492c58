"""CPU: the rule that picks the small-batch linear kernel's tile (pc3d_linear_tile, include/pc3d.h) over a grid of layer
shapes: it names a form that exists, never takes a layer past 256 workgroups (one per CU) that the 32x16 form keeps
within them, and is a function of (B, K, O) alone. No kernel runs."""
import itertools

BS = (1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 48, 64, 100, 128, 256, 512)
KS = (16, 64, 128, 144, 256, 512, 1024)
OS = (64, 72, 128, 200, 256, 512, 520, 1024, 2048, 4096)


def _wgs(form, B, O):
    tr, tc = (int(v) for v in form.split("x"))
    return -(-O // tc) * -(-B // tr)


def test_rule_names_a_form_and_keeps_the_layer_within_the_cus(ops):
    assert set(ops.LINEAR_TILES) == {"32x16", "16x16", "16x8", "8x8"}
    assert sorted(ops.LINEAR_TILES.values()) == [1, 2, 3, 4]
    lib = ops._lib.load()
    for B, K, O in itertools.product(BS, KS, OS):
        n = lib.pc3d_linear_tile(B, K, O)
        assert n in ops.LINEAR_TILES.values(), (B, K, O, n)
        form = ops.linear_tile(B, K, O)
        assert ops.LINEAR_TILES[form] == n
        if _wgs("32x16", B, O) <= 256:
            assert _wgs(form, B, O) <= 256, (B, K, O, form)


def test_rule_is_a_function_of_its_arguments(ops):
    lib = ops._lib.load()
    grid = list(itertools.product(BS, KS, OS))
    first = [lib.pc3d_linear_tile(*s) for s in grid]
    again = [lib.pc3d_linear_tile(*s) for s in reversed(grid)][::-1]      # another call order, the same answers
    assert first == again


def test_tile_argument_of_the_ops_functions_is_checked_before_any_launch(ops):
    import pytest
    for bad in ("64x64", 2, "16X16"):
        with pytest.raises(ValueError):
            ops._linear_tile("linear", bad)
    assert ops._linear_tile("linear", None) == 0

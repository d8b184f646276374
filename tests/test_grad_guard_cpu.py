"""The host side of the gradient norm / clipping / non-finite guard (no kernel runs):

  * the range table the optimizer builds from a small policy's ParamStore and the workspace's five parts
    (encoder, decoder, video_head, action_head, rest) covers every element of every group range exactly
    once, and the padding between the groups is in no range;
  * uva_grad_norm_workspace_bytes answers without a device;
  * uva_grad_sumsq refuses more than 64 ranges, more than 16 slots and a range outside the buffer with
    hipErrorInvalidValue, from its host-side argument checks (before any launch)."""
import ctypes

import pytest
import torch

import replay

HIP_ERROR_INVALID_VALUE = 1


@pytest.fixture
def fp32():
    from unified_video_action_amd.runtime import RT
    RT.set_precision("fp32")
    yield
    RT.set_precision("bf16")


def _parts(mar):
    return {"encoder": [mar.encoder_blocks], "decoder": [mar.decoder_blocks],
            "video_head": [getattr(mar, "diffloss", None), getattr(mar, "diffloss_wrist", None)],
            "action_head": [getattr(mar, "diffactloss", None), getattr(mar, "diffproploss", None)]}


def test_range_table_covers_every_group_element_once(fp32):
    from unified_video_action_amd.workspace.optim import grad_range_table
    pol = replay.golden_policy()
    opt = pol.get_optimizer(weight_decay=0.02, learning_rate=1e-4, betas=(0.9, 0.95))
    st = opt.store
    names, table = grad_range_table(st, _parts(pol.model))
    assert names == ["encoder", "decoder", "video_head", "action_head", "rest"]
    assert len(table) <= 64
    cnt = torch.zeros(st.total, dtype=torch.int32)
    for o, k, slot in table:
        assert 0 <= slot < len(names) and k > 0 and 0 <= o and o + k <= st.total
        cnt[o:o + k] += 1
    in_group = torch.zeros(st.total, dtype=torch.bool)
    for o, k in st.group_ranges:
        in_group[o:o + k] = True
    assert st.n_params == int(in_group.sum()) < st.total  # the layout does pad between / after the groups
    assert torch.equal(cnt[in_group], torch.ones(int(in_group.sum()), dtype=torch.int32))
    assert int(cnt[~in_group].sum()) == 0
    # each named part holds exactly its own parameters; every part of this policy is non-empty
    for slot, (name, objs) in enumerate(_parts(pol.model).items()):
        want = sum(p.numel() for o in objs if o is not None for p in o.parameters())
        assert want > 0 and sum(k for _, k, s in table if s == slot) == want, name
    assert sum(k for _, k, s in table if s == 4) > 0

    # the optimizer builds the same table from the same parts; unset switches the pass off again
    opt.set_grad_guard(grad_norm_parts=_parts(pol.model))
    assert opt.grad_part_names == names and opt._guard["table"] == table
    opt.set_grad_guard()
    assert opt._guard is None and opt.grad_part_names == [] and opt.grad_stats() == {}
    with pytest.raises(ValueError):
        grad_range_table(st, {"a": [pol.model.encoder_blocks], "b": [pol.model.encoder_blocks[0]]})


def test_workspace_bytes_is_a_host_query():
    from unified_video_action_amd.native import ops
    chunk = ops.grad_norm_chunk_elems()
    assert chunk > 0 and chunk % 4 == 0
    for n, r in ((0, 0), (1, 1), (chunk, 1), (260_000_000, 64)):
        b = ops.grad_norm_workspace_bytes(n, r)
        assert b >= 8 * (-(-n // chunk) + r) and b % 8 == 0  # one fp64 partial per chunk, ranges may split chunks
    assert ops.grad_norm_workspace_bytes(260_000_000, 64) < 1 << 20
    with pytest.raises(ValueError):
        ops.grad_norm_workspace_bytes(100, 65)
    assert ops.grad_norm_chain_len(chunk * 256, 1) == ops.grad_norm_chain_len(1, 1) + 1


def test_launcher_refuses_bad_tables_on_the_host():
    """the argument checks run before any launch (and before any pointer is looked at): dummy non-null
    pointers, no device needed"""
    from unified_video_action_amd.native import ops
    from unified_video_action_amd.native.lib import lib
    n_total = 1 << 20
    dummy = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(dummy)

    def launch(ranges, n_ranges, n_slots):
        table = ops.range_table(ranges)
        return lib().query("uva_grad_sumsq", ptr, n_total, ctypes.addressof(table), n_ranges, n_slots, ptr, ptr,
                           1 << 20, None)

    ok = [(i * 16, 16, 0) for i in range(65)]
    assert launch(ok, 65, 1) == HIP_ERROR_INVALID_VALUE                      # more than 64 ranges
    assert launch(ok[:4], 4, 17) == HIP_ERROR_INVALID_VALUE                  # more than 16 slots
    assert launch(ok[:4], 4, 0) == HIP_ERROR_INVALID_VALUE
    assert launch([(n_total - 8, 9, 0)], 1, 1) == HIP_ERROR_INVALID_VALUE    # runs past the end
    assert launch([(-1, 4, 0)], 1, 1) == HIP_ERROR_INVALID_VALUE
    assert launch([(0, -4, 0)], 1, 1) == HIP_ERROR_INVALID_VALUE
    assert launch([(n_total + 1, 0, 0)], 1, 1) == HIP_ERROR_INVALID_VALUE
    assert launch([(0, 16, 1)], 1, 1) == HIP_ERROR_INVALID_VALUE             # slot outside [0, n_slots)
    # a table that is fine, with a workspace too small for its chunks: refused as well
    table = ops.range_table([(0, n_total, 0)])
    assert lib().query("uva_grad_sumsq", ptr, n_total, ctypes.addressof(table), 1, 1, ptr, ptr, 8, None) \
        == HIP_ERROR_INVALID_VALUE
    with pytest.raises(RuntimeError):
        lib().call("uva_grad_guard", ptr, 17, 1.0, 1.0, 0, ptr, None)
    with pytest.raises(RuntimeError):
        lib().call("uva_adamw_ema_guarded", ptr, ptr, ptr, ptr, None, None, 4, 0, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1, 1.0,
                   0.0, None, None)

"""CPU: the prompt schedule of `fifo_ddim_sampling_multiprompts` (funcs.py:375-468) against a plain restatement of the reference's
rule, the multi-prompt file layout, and the calls the loop refuses before it touches a device."""
import types

import numpy as np
import pytest
import torch


def _reference_segments(multiprompts, S, f, n=None):
    """funcs.py:379,420-427 restated: the segment index j at every outer iteration"""
    prompt_lengths = np.array([int(i) for i in multiprompts[-1].split(',')]).cumsum()
    out, j = [], 0
    for i in range(prompt_lengths[-1] + S - f if n is None else n):
        if i - (S - f) >= prompt_lengths[j]:
            j = j + 1
        out.append(j)
    return out


def _args(S=16, f=8, lookahead=True):
    return types.SimpleNamespace(num_inference_steps=S, video_length=f, lookahead_denoising=lookahead, num_partitions=S // f,
                                 new_video_length=10)


def _mp(counts):
    return [f"prompt {k}" for k in range(len(counts.split(",")))] + [counts]


@pytest.mark.parametrize("counts", ["40,60", "2,3", "3,0,2", "0,5", "5", "2,0,0,4", "1,1,1,1", "4,0"])
@pytest.mark.parametrize("S,f", [(64, 16), (16, 8), (8, 8)])
@pytest.mark.parametrize("lookahead", [True, False])
def test_segment_schedule_is_the_reference_rule(counts, S, f, lookahead):
    from moca_video_amd.fifo import multiprompt_segments
    mp = _mp(counts)
    seg = multiprompt_segments(_args(S, f, lookahead), mp)
    assert seg == _reference_segments(mp, S, f)
    assert len(seg) == sum(int(c) for c in counts.split(",")) + S - f
    assert all(j == 0 for j in seg[:S - f]), "the S - f warm-up iterations stay on the first prompt"
    assert all(b - a in (0, 1) for a, b in zip(seg, seg[1:])), "j moves by at most one per iteration"


def test_segment_schedule_quirks():
    from moca_video_amd.fifo import multiprompt_segments
    a = _args(16, 8)
    # a segment of 0 frames still lasts one iteration; a trailing one is never reached
    assert multiprompt_segments(a, _mp("2,0,3")) == [0] * 10 + [1] + [2] * 2
    assert multiprompt_segments(a, _mp("3,0")) == [0] * 11
    assert multiprompt_segments(a, _mp("0,2")) == [0] * 8 + [1] * 2
    # the trange cut: a prefix of the schedule; running past the last prompt is where the reference fails on an index
    assert multiprompt_segments(a, _mp("2,3"), n_iterations=12) == _reference_segments(_mp("2,3"), 16, 8, 12) == [0] * 10 + [1] * 2
    with pytest.raises(ValueError, match="past the last prompt"):
        multiprompt_segments(a, _mp("2,3"), n_iterations=14)
    with pytest.raises(ValueError, match="frame counts"):
        multiprompt_segments(a, ["one prompt", "two prompt", "5"])


def test_load_multiprompts_round_trips_the_reference_layout(tmp_path):
    from moca_video_amd.io import load_multiprompts
    mp = ["a cat walks on the grass", "a cat jumps, then lands on a wall", "40,60"]
    p = tmp_path / "multiprompts.txt"
    p.write_text("\n".join(mp) + "\n")
    assert load_multiprompts(str(p)) == mp
    p.write_text("  a cat walks \n\na cat jumps\n 1, 2 \n")
    assert load_multiprompts(str(p)) == ["a cat walks", "a cat jumps", "1,2"]
    for bad in ("a\nb\n1\n", "a\n1,x\n", "40\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            load_multiprompts(str(p))


class _Model:
    """what the loop reads of a model before it touches a device"""
    def __init__(self, image_attention=False):
        self.model = types.SimpleNamespace(diffusion_model=types.SimpleNamespace(use_image_attention=image_attention))
        self.cond_stage_model = None
        self.uncond_type = "zero_embed"


@pytest.mark.parametrize("kw", ["davis_data", "davis_masks"])
def test_refuses_davis_inputs(kw):
    from moca_video_amd.fifo import fifo_ddim_sampling_multiprompts
    with pytest.raises(NotImplementedError, match=kw):
        fifo_ddim_sampling_multiprompts(_args(), _Model(), {}, [1, 4, 8, 16, 16], None, _mp("2,3"), 12.0, **{kw: torch.zeros(1)})


def test_refuses_image_attention_model():
    from moca_video_amd.fifo import fifo_ddim_sampling_multiprompts
    with pytest.raises(NotImplementedError, match="image-attention"):
        fifo_ddim_sampling_multiprompts(_args(), _Model(image_attention=True), {}, [1, 4, 8, 16, 16], None, _mp("2,3"), 12.0,
                                        embeds=[torch.zeros(1, 77, 128)] * 2, uc_emb=torch.zeros(1, 77, 128))


def test_needs_the_embeddings_without_a_text_encoder():
    """no text encoder: the prompt embeddings come as `embeds`, the empty prompt's as `uc_emb` (whatever `uncond_type` says)"""
    from moca_video_amd.fifo import fifo_ddim_sampling_multiprompts
    run = lambda **kw: fifo_ddim_sampling_multiprompts(_args(), _Model(), {}, [1, 4, 8, 16, 16], None, _mp("2,3"), 12.0, **kw)
    with pytest.raises(ValueError, match="embeds"):
        run(uc_emb=torch.zeros(1, 77, 128))
    with pytest.raises(ValueError, match="uc_emb"):
        run(embeds=[torch.zeros(1, 77, 128)] * 2)
    with pytest.raises(ValueError, match="2 prompts"):
        run(embeds=[torch.zeros(1, 77, 128)] * 3, uc_emb=torch.zeros(1, 77, 128))
    with pytest.raises(ValueError, match="decode"):
        run(embeds=[torch.zeros(1, 77, 128)] * 2, uc_emb=torch.zeros(1, 77, 128), save_frames=True, output_dir="out")


def test_set_context_refuses_another_token_count():
    """the plan's context segments are fixed: a prompt switch replaces the conditional rows, it cannot change their number"""
    from moca_video_amd.fifo_graph import FifoEngine
    eng = FifoEngine.__new__(FifoEngine)
    eng.plan = types.SimpleNamespace(segs=[(4, 77), (4, 77)])
    with pytest.raises(ValueError, match="77"):
        eng.set_context(torch.zeros(1, 154, 128))
    with pytest.raises(ValueError, match="77"):
        eng.set_context([torch.zeros(1, 77, 128), torch.zeros(1, 77, 128)])        # MoCA's two-prompt context
    with pytest.raises(ValueError):
        eng.set_context(torch.zeros(2, 77, 128))

"""SamMaskDecoderEngine / SamPredictorEngine without a GPU: the numpy rule (tests/sam_decoder_rule.py) against transformers' float64 module and against
the golden, the key maps of both state-dict layouts, every refusal (all before any launch), the host-side size and coordinate arithmetic, the
`sam_predictor` arm of do_segmentation with a recording stub, the opt-in drop-in, and the new C-ABI symbols."""
import ctypes
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load('make_sam_decoder_golden')
GE = _load('make_sam_encoder_golden')
sys.path.insert(0, HERE)
import sam_decoder_rule as R  # noqa: E402


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def rule(case, variant=None):
    inp = G.make_inputs(case)
    return R.decoder_forward(G.make_weights(case, variant), G.config_dict(case), inp['embedding'], inp['boxes'], inp['points'], inp['labels'])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['A', 'B', 'C'])
def test_numpy_rule_is_the_golden(case):
    """the rule, run from the regenerated weights and inputs, reproduces every tap the golden stores from transformers' float64 module -- to the float32
    the golden is stored in"""
    ref, inp = np.load(G.REF), G.make_inputs(case)
    assert str(ref[f'{case}.weights_sha256']) == G.digest(G.make_weights(case)) and str(ref[f'{case}.inputs_sha256']) == G.digest(inp)
    taps = rule(case)
    for n in G.tap_names(case):
        assert tuple(ref[f'{case}.{n}.shape']) == taps[n].shape, n
        assert rel_l2(taps[n].reshape(-1)[G.sample_index(case, n, taps[n].size)], ref[f'{case}.{n}']) < 1e-6, n
    for v in G.variants(case):
        low = rule(case, v)['low_res_masks']
        assert rel_l2(low.reshape(-1)[G.sample_index(case, 'low_res_masks', low.size)], ref[f'{case}.{v}.low_res_masks']) < 1e-6, v
        assert float(ref[f'{case}.{v}.change']) > 1e-3
    assert float(ref[f'{case}.conditioning.moved_by_1e-3']) <= 1e-2 and float(ref[f'{case}.conditioning.fp32_module']) <= 1e-5


@pytest.mark.parametrize('case', ['B', 'C'])
def test_numpy_rule_is_transformers_float64_module(case):
    pytest.importorskip('transformers')
    ref = G.run_module(G.build_module(case, torch.float64), G.make_inputs(case))
    taps = rule(case)
    for n in G.tap_names(case):
        assert rel_l2(taps[n], ref[n]) < 1e-9, n


def test_rule_postprocess_is_two_interpolations():
    """against torch's float32 F.interpolate, which computes the scale in fp32 as the rule does (its float64 kernel takes the scale in double and sits 1e-6 away)"""
    import torch.nn.functional as F
    low = np.random.RandomState(0).standard_normal((1, 2, 48, 48)).astype(np.float32)
    want = F.interpolate(F.interpolate(torch.from_numpy(low), (192, 192), mode='bilinear', align_corners=False)[..., :144, :192], (150, 200), mode='bilinear', align_corners=False)
    assert rel_l2(R.postprocess(low, 192, 144, 192, 150, 200), want.numpy()) < 5e-7


# ---- key maps -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dec(lib):
    from mvedit_amd.sam import SamMaskDecoderEngine
    return SamMaskDecoderEngine(G.config_dict('A'), device='cpu')


def test_key_maps_of_both_layouts(dec):
    sd = G.make_weights('A')
    assert sorted(dec.expected_parameters()) == sorted(sd) and len(set(dec.expected_parameters())) == len(sd)
    tf = dec.map_state_dict(sd)
    sa_sd = G.segment_anything_keys(sd)
    sa = dec.map_state_dict(sa_sd)
    assert sorted(tf) == sorted(sa) == sorted(sd)
    for k in sd:
        assert tf[k] is sd[k] and sa[k] is sd[k], k
    # segment_anything's own spellings, restated from its published source
    for k in ('prompt_encoder.pe_layer.positional_encoding_gaussian_matrix', 'prompt_encoder.point_embeddings.3.weight', 'mask_decoder.transformer.layers.1.norm4.bias',
              'mask_decoder.transformer.norm_final_attn.weight', 'mask_decoder.output_upscaling.0.weight', 'mask_decoder.output_upscaling.1.bias',
              'mask_decoder.output_upscaling.3.weight', 'mask_decoder.output_hypernetworks_mlps.3.layers.2.weight', 'mask_decoder.iou_prediction_head.layers.0.bias'):
        assert k in sa_sd, k
    # the mask_input path's parameters and transformers' tied copy are accepted by name and left out
    extra = dict(sd)
    extra.update({'prompt_encoder.mask_embed.conv1.weight': 0, 'prompt_encoder.mask_embed.layer_norm2.bias': 0, 'prompt_encoder.shared_embedding.positional_embedding': 0})
    assert sorted(dec.map_state_dict(extra)) == sorted(sd)
    extra = dict(sa_sd)
    extra.update({'prompt_encoder.mask_downscaling.0.weight': 0, 'prompt_encoder.mask_downscaling.6.bias': 0})
    assert sorted(dec.map_state_dict(extra)) == sorted(sd)
    with pytest.raises(KeyError, match='mask_decoder.transformer.layers.2.norm1.weight'):
        dec.map_state_dict(dict(sa_sd, **{'mask_decoder.transformer.layers.2.norm1.weight': 0}))
    with pytest.raises(KeyError, match="'image_encoder.pos_embed'"):
        dec.map_state_dict(dict(sd, **{'image_encoder.pos_embed': 0}))
    with pytest.raises(KeyError, match='another key already filled'):
        dec.map_state_dict(dict(sa_sd, **{'mask_decoder.upscale_conv1.weight': 0}))
    with pytest.raises(KeyError, match='is missing'):
        dec.load_state_dict({k: v for k, v in sd.items() if k != 'mask_decoder.iou_token.weight'})


class _Attn(torch.nn.Module):
    def __init__(self, C, inner, sa):
        super().__init__()
        setattr(self, 'num_heads' if sa else 'num_attention_heads', 8)
        self.q_proj = torch.nn.Linear(C, inner)


def _sam_like(sa, eps, eps_final):
    """stand-in with what from_module reads off a segment_anything `Sam` / transformers `SamModel`"""
    C = 256
    m, pe, md, tf = torch.nn.Module(), torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
    if sa:
        pe.pe_layer = torch.nn.Module()
    pe.image_embedding_size, pe.input_image_size = (16, 16), ((256, 256) if sa else 256)
    md.iou_token, md.mask_tokens = torch.nn.Embedding(1, C), torch.nn.Embedding(4, C)
    tf.layers = torch.nn.ModuleList()
    for _ in range(2):
        layer = torch.nn.Module()
        layer.self_attn, layer.cross_attn_token_to_image = _Attn(C, C, sa), _Attn(C, C // 2, sa)
        setattr(layer, 'norm1' if sa else 'layer_norm1', torch.nn.LayerNorm(C, eps=eps))
        layer.mlp = torch.nn.Module()
        layer.mlp.lin1 = torch.nn.Linear(C, 2048)
        tf.layers.append(layer)
    setattr(tf, 'norm_final_attn' if sa else 'layer_norm_final_attn', torch.nn.LayerNorm(C, eps=eps_final))
    md.transformer, head = tf, torch.nn.Module()
    head.layers = torch.nn.ModuleList([torch.nn.Linear(C, C) for _ in range(3 if sa else 1)])
    head.proj_in = torch.nn.Linear(C, C)
    md.iou_prediction_head = head
    m.prompt_encoder, m.mask_decoder = pe, md
    return m


@pytest.mark.parametrize('sa,eps,eps_final', [(True, 1e-5, 1e-5), (False, 1e-6, 1e-5)])
def test_from_module_reads_both_eps_values_off_the_module(lib, sa, eps, eps_final):
    from mvedit_amd.sam import SamMaskDecoderEngine
    eng = SamMaskDecoderEngine.from_module(_sam_like(sa, eps, eps_final))
    assert eng.cfg == dict(G.config_dict('A'), layer_norm_eps=eps, final_layer_norm_eps=eps_final) and eng.device.type == 'cpu'
    with pytest.raises(TypeError, match='neither a Sam nor a SamModel'):
        SamMaskDecoderEngine.from_module(torch.nn.Linear(2, 2))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refused_at_create(lib):
    from mvedit_amd.sam import SamMaskDecoderEngine
    with pytest.raises(NotImplementedError, match='attention_downsample_rate 4'):
        SamMaskDecoderEngine(dict(G.config_dict('A'), attention_downsample_rate=4), device='cpu')
    with pytest.raises(NotImplementedError, match='head dims 32'):
        SamMaskDecoderEngine(dict(G.config_dict('A'), num_attention_heads=4), device='cpu')
    with pytest.raises(NotImplementedError, match='head dims 32'):
        SamMaskDecoderEngine(dict(G.config_dict('A'), hidden_size=192), device='cpu')
    with pytest.raises(lib.MveError, match='iou head of depth 4'):
        SamMaskDecoderEngine(dict(G.config_dict('A'), iou_head_depth=4), device='cpu')
    with pytest.raises(ValueError, match='mlp_dim is missing'):
        SamMaskDecoderEngine({k: v for k, v in G.config_dict('A').items() if k != 'mlp_dim'}, device='cpu')


def test_decoder_refusals_before_any_launch(dec):
    emb = torch.zeros(1, 256, 16, 16)
    with pytest.raises(NotImplementedError, match='inference only'):
        dec.train()
    assert dec.train(False) is dec and dec.eval() is dec and dec.requires_grad_(False) is dec
    with pytest.raises(NotImplementedError, match='inference only'):
        dec.requires_grad_(True)
    with pytest.raises(ValueError, match='no prompt at all'):
        dec.run(emb)
    with pytest.raises(ValueError, match=r'not \[B, 256, 16, 16\]'):
        dec.run(torch.zeros(1, 256, 12, 12), torch.zeros(1, 1, 4))
    with pytest.raises(ValueError, match='unequal shape'):
        dec.run(emb, torch.zeros(1, 2, 4), torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'not \[B = 1, P, 4\]'):
        dec.run(emb, torch.zeros(2, 1, 4))
    with pytest.raises(ValueError, match='does not match the points'):
        dec.run(emb, None, torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match='come together'):
        dec.run(emb, None, torch.zeros(1, 1, 2, 2))
    with pytest.raises(ValueError, match=r'outside \{-1, 0, 1\}'):
        dec.run(emb, None, torch.zeros(1, 1, 2, 2), torch.tensor([[[1, 2]]]))
    assert dec.n_tokens(9, True) == 16 and dec.n_tokens(10, False) == 16 and dec.n_tokens(0, True) == 7 and dec.n_tokens(3, False) == 9
    with pytest.raises(NotImplementedError, match='17 tokens'):
        dec.run(emb, torch.zeros(1, 1, 4), torch.zeros(1, 1, 10, 2), torch.zeros(1, 1, 10, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match='17 tokens'):
        dec.run(emb, None, torch.zeros(1, 1, 11, 2), torch.zeros(1, 1, 11, dtype=torch.int32))


def _predictor(lib, dec):
    from mvedit_amd.sam import SamImageEncoderEngine, SamPredictorEngine
    enc = SamImageEncoderEngine(GE.config_dict('A'), torch.float16, 'cpu')
    return SamPredictorEngine(enc, dec, mask_threshold=0.0)


def test_predictor_surface_and_refusals(lib, dec):
    from mvedit_amd.sam import SamImageEncoderEngine, SamPredictorEngine
    p = _predictor(lib, dec)
    assert p.is_image_set is False and p.features is None and p.original_size is None and p.input_size is None and p.device.type == 'cpu'
    assert p.model.image_encoder is p.encoder and p.model.mask_threshold == 0.0 and p.model.image_format == 'RGB'
    for call in (lambda: p.predict(box=np.array([1, 2, 3, 4])), lambda: p.predict_torch(boxes=torch.zeros(1, 4)), p.get_image_embedding):
        with pytest.raises(ValueError, match='An image must be set'):
            call()
    with pytest.raises(ValueError, match='uint8'):
        p.set_image(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match='image_format'):
        p.set_image(np.zeros((8, 8, 3), np.uint8), 'HSV')
    # as after set_image of a 150 x 200 image (no launch: the refusals below come first)
    p.features, p.original_size, p.input_size, p.is_image_set = torch.zeros(1, 256, 16, 16), (150, 200), (192, 256), True
    with pytest.raises(NotImplementedError, match='mask_input'):
        p.predict(box=np.array([1, 2, 3, 4]), mask_input=np.zeros((1, 64, 64)))
    with pytest.raises(NotImplementedError, match='mask_input'):
        p.predict_torch(boxes=torch.zeros(1, 4), mask_input=torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError, match='no prompt at all'):
        p.predict()
    with pytest.raises(ValueError, match='point_labels must be supplied'):
        p.predict(point_coords=np.zeros((2, 2)))
    with pytest.raises(ValueError, match=r'outside \{-1, 0, 1\}'):
        p.predict(point_coords=np.zeros((2, 2)), point_labels=np.array([1, 3]))
    with pytest.raises(ValueError, match='unequal shape'):
        p.predict_torch(point_coords=torch.zeros(2, 1, 2), point_labels=torch.zeros(2, 1, dtype=torch.int32), boxes=torch.zeros(3, 4))
    with pytest.raises(NotImplementedError, match='17 tokens'):
        p.predict(point_coords=np.zeros((11, 2)), point_labels=np.ones(11, np.int64))
    p.reset_image()
    assert p.is_image_set is False and p.features is None
    with pytest.raises(ValueError, match='do not fit together'):
        SamPredictorEngine(SamImageEncoderEngine(GE.config_dict('B'), torch.float16, 'cpu'), dec)
    with pytest.raises(ValueError, match='the decoder reads'):
        SamPredictorEngine(SamImageEncoderEngine(GE.config_dict('A'), torch.bfloat16, 'cpu'), dec)


# ---- host-side arithmetic -------------------------------------------------------------------------------------------------------------------------------
def test_preprocess_shape_and_coordinates(lib, dec):
    from mvedit_amd.sam import preprocess_shape
    sizes = [(150, 200), (200, 150), (1024, 1024), (768, 1024), (333, 1000), (1, 7), (2047, 1365), (480, 640), (641, 480)]
    for h, w in sizes:
        for S in (256, 1024):
            nh, nw = preprocess_shape(h, w, S)
            scale = S * 1.0 / max(h, w)
            assert (nh, nw) == (int(h * scale + 0.5), int(w * scale + 0.5)) and max(nh, nw) == S
    try:
        from transformers import SamImageProcessor
        ip = SamImageProcessor()
        for h, w in sizes:
            assert tuple(ip._get_preprocess_shape((h, w), 1024)) == preprocess_shape(h, w, 1024), (h, w)
    except ImportError:
        pass
    p = _predictor(lib, dec)
    p.original_size, p.input_size = (150, 200), preprocess_shape(150, 200, 256)
    assert p.input_size == (192, 256)
    pts = np.array([[10.0, 20.0], [199.0, 149.0]])
    got = p.apply_coords(pts)
    assert np.array_equal(got, pts * np.array([256 / 200, 192 / 150])) and got is not pts and pts[0, 0] == 10.0
    box = p.apply_coords(np.array([10, 20, 110, 140]).reshape(2, 2)).reshape(4)
    assert np.array_equal(box, np.array([10 * 1.28, 20 * 1.28, 110 * 1.28, 140 * 1.28]))


# ---- do_segmentation ------------------------------------------------------------------------------------------------------------------------------------
class Seg(torch.nn.Module):
    """the stand-in segmentor of tests/test_segmentor.py"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.6, -0.2, 0.4]))

    def forward(self, x):
        return torch.sigmoid((x * self.w.view(1, 3, 1, 1)).sum(1, keepdim=True) * 3 - 1)


class RecordingPredictor:
    def __init__(self):
        self.calls = []

    def set_image(self, image):
        self.calls.append(('set_image', image.copy()))
        self.hw = image.shape[:2]

    def predict(self, box=None, multimask_output=None, **kw):
        assert not kw
        self.calls.append(('predict', np.array(box), multimask_output))
        masks = np.zeros((3,) + self.hw, bool)
        masks[0] = True
        masks[2, box[1]:box[3], box[0]:box[2]] = True        # the LAST mask is the one that is kept
        return masks, np.zeros(3), np.zeros((3, 64, 64))


def _images():
    x = torch.rand(3, 3, 20, 24, generator=torch.Generator().manual_seed(0))
    x[0, :, :8] = 1.0
    return x


def test_do_segmentation_without_a_predictor_is_unchanged():
    from mvedit_amd.pipelines.utils import do_segmentation
    g = np.load(os.path.join(HERE, 'golden', 'segmentation_ref.npz'))
    with torch.no_grad():
        for i, (pad, bg) in enumerate(((0, None), (4, None), (3, (1.0, 1.0, 1.0)))):
            assert torch.equal(do_segmentation(_images(), Seg(), padding=pad, bg_color=bg, sam_predictor=None, sam_erosion=0), torch.from_numpy(g[f'case{i}']))
            assert torch.equal(do_segmentation(_images(), Seg(), pad, bg), torch.from_numpy(g[f'case{i}']))


def test_do_segmentation_with_a_recording_predictor():
    import inspect
    from mvedit_amd.pipelines.utils import do_segmentation
    assert list(inspect.signature(do_segmentation).parameters) == ['in_imgs', 'seg_model', 'padding', 'bg_color', 'color_threshold', 'sam_predictor', 'sam_erosion']
    x, seg, rec = _images(), Seg(), RecordingPredictor()
    with torch.no_grad():
        tracer = seg(x)
        out = do_segmentation(x, seg, sam_predictor=rec)
    assert out.shape == (3, 4, 20, 24) and out.dtype == x.dtype and torch.equal(out[:, :3], x)
    assert [c[0] for c in rec.calls] == ['set_image', 'predict'] * 3
    for i in range(3):
        img, (_, box, multi) = rec.calls[2 * i][1], rec.calls[2 * i + 1]
        assert img.dtype == np.uint8 and np.array_equal(img, (x[i].permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()) and multi is True
        fg = (tracer[i, 0] > 0.5).numpy()
        ys, xs = np.nonzero(fg.any(1))[0], np.nonzero(fg.any(0))[0]
        assert box.tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        want = np.zeros((20, 24), np.float32)
        want[box[1]:box[3], box[0]:box[2]] = 1
        assert np.array_equal(out[i, 3].numpy(), want)
    # the background-colour rule: pixels further than the threshold from bg_color are foreground whatever SAM says
    with torch.no_grad():
        out = do_segmentation(x, seg, bg_color=(1.0, 1.0, 1.0), sam_predictor=RecordingPredictor())
    img = (x.permute(0, 2, 3, 1) * 255).round().numpy()
    near = np.all((255 - 0.25 * 255 <= img) & (img <= 255 + 0.25 * 255), axis=-1)
    assert bool(out[:, 3].numpy()[~near].all()) and not out[0, 3, :8].numpy()[:min(8, int(rec.calls[1][1][1]))].any()
    with pytest.raises(NotImplementedError, match='sam_erosion'):
        do_segmentation(x, seg, sam_predictor=rec, sam_erosion=2)
    with pytest.raises(ValueError, match='no foreground in image 0'):
        do_segmentation(x, lambda t: torch.zeros(t.shape[0], 1, *t.shape[2:]), sam_predictor=rec)


# ---- drop-in ------------------------------------------------------------------------------------------------------------------------------------------
def test_swap_sam_predictor_is_opt_in_and_undone(lib, dec, monkeypatch):
    from mvedit_amd import dropin
    from mvedit_amd.sam import SamPredictorEngine
    made = []
    eng = _predictor(lib, dec)
    monkeypatch.setattr(SamPredictorEngine, 'from_predictor', classmethod(lambda cls, p: made.append(p) or eng))
    torch_predictor = SimpleNamespace(model=SimpleNamespace(image_encoder=torch.nn.Linear(2, 2)))
    runner = SimpleNamespace(predictor=torch_predictor)
    dropin.swap_engines(runner)
    dropin.install()
    try:
        assert runner.predictor is torch_predictor and not made                    # neither the default swap nor install() touches the predictor
    finally:
        dropin.uninstall()
    empty = SimpleNamespace(predictor=None)
    assert dropin.swap_sam_predictor(empty) is empty and empty.predictor is None
    assert dropin.swap_sam_predictor(runner) is runner and runner.predictor is eng and made == [torch_predictor]
    dropin.swap_sam_predictor(runner)                                              # idempotent
    assert runner.predictor is eng and len(made) == 1
    dropin.uninstall()
    assert runner.predictor is torch_predictor
    dropin.swap_sam_predictor(runner)                                              # the engine is cached on the source predictor
    assert runner.predictor is eng and len(made) == 1
    dropin.uninstall()
    assert runner.predictor is torch_predictor and callable(dropin.swap_sam_image_encoder)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------------------------
ARITY = dict(mve_sam_preprocess=9, mve_sam_dense_pe=5, mve_sam_prompt_tokens=16, mve_sam_src=9, mve_gemm_f32=14, mve_attention_f32=15, mve_layernorm_f32=8,
             mve_add_rows_f32=7, mve_sam_upscale=14, mve_sam_token_mlps=16, mve_sam_mask_product=8, mve_sam_postprocess=12, mve_sam_decoder_create=14,
             mve_sam_decoder_finalize=2, mve_sam_decoder_plan=8, mve_sam_decoder_forward=15, mve_sam_decoder_destroy=1)


def test_new_symbols_are_exported_with_the_declared_arity(lib):
    for name, n in ARITY.items():
        assert name in lib.PROTOS and len(lib.PROTOS[name][1]) == n, name
        assert lib.raw(name) is not None and len(lib.raw(name).argtypes) == n


def test_argument_errors_come_before_the_device(lib, dec):
    f, p = ctypes.c_float, ctypes.c_void_p(4096)

    def bad(name, *args, match, code=-1):
        assert lib.raw(name)(*args) == code and match in lib.last_error(), (name, lib.last_error())
    bad('mve_gemm_f32', None, 8, p, 8, None, None, 0, p, 8, 1, 8, 8, 0, None, match='null')
    bad('mve_gemm_f32', p, 4, p, 8, None, None, 0, p, 8, 1, 8, 8, 0, None, match='leading dimension')
    bad('mve_gemm_f32', p, 8, p, 8, None, None, 0, p, 8, 0, 8, 8, 0, None, match='bad shape')
    bad('mve_attention_f32', p, 128, p, 128, p, 128, p, 128, 1, 4, 4, 8, 24, f(1.0), None, match='head_dim 24')
    bad('mve_attention_f32', p, 130, p, 128, p, 128, p, 128, 1, 4, 4, 8, 16, f(1.0), None, match='multiples of 4')
    bad('mve_attention_f32', ctypes.c_void_p(4100), 128, p, 128, p, 128, p, 128, 1, 4, 4, 8, 16, f(1.0), None, match='aligned')
    bad('mve_attention_f32', p, 128, p, 128, p, 128, p, 128, 1, 4, 0, 8, 16, f(1.0), None, match='Lk 0')
    bad('mve_sam_prompt_tokens', None, None, None, 1, 0, p, p, p, p, p, 4, 256, f(256.0), p, 5, None, match='no prompt')
    bad('mve_sam_prompt_tokens', p, None, None, 1, 0, p, p, p, p, p, 4, 256, f(256.0), p, 9, None, match='the prompt has 7 tokens')
    bad('mve_sam_prompt_tokens', p, p, p, 1, 10, p, p, p, p, p, 4, 256, f(256.0), p, 17, None, match='exceed 16')
    bad('mve_sam_src', 0, p, p, p, 2, 2, 256, 16, None, match='dtype')
    bad('mve_sam_src', 1, p, p, p, 3, 2, 256, 16, None, match='bad arguments')
    bad('mve_sam_upscale', p, p, p, None, None, f(1e-6), p, p, 1, 16, 256, 64, 1, None, match='LayerNorm2d parameters')
    bad('mve_sam_upscale', p, p, p, p, p, f(1e-6), p, p, 1, 16, 256, 64, 3, None, match='mode 3')
    bad('mve_sam_token_mlps', p, 1, 4, 256, 256, 32, 4, p, p, p, p, p, p, p, p, None, match='bad N 1 / T 4')
    bad('mve_sam_token_mlps', p, 1, 7, 1024, 256, 32, 4, p, p, p, p, p, p, p, p, None, match='at most 512')
    bad('mve_sam_mask_product', p, p, p, 1, 8, 128, 100, None, match='at most 512')
    bad('mve_sam_preprocess', 1, p, 300, 200, 256, None, None, p, None, match='does not fit')
    bad('mve_sam_preprocess', 1, p, 100, 200, 256, None, (f * 3)(1, 0, 1), p, None, match='pixel_std')
    bad('mve_sam_postprocess', p, 3, 64, 256, 300, 256, 10, 10, f(0.0), p, None, None, match='bad shape')
    bad('mve_sam_dense_pe', p, p, 16, 255, None, match='bad arguments')
    h = ctypes.c_void_p()
    bad('mve_sam_decoder_create', ctypes.byref(h), 1, 256, 2, 8, 2048, 4, 256, 3, 1, 64, 1024, f(1e-6), f(1e-5), match='attention_downsample_rate 1')
    bad('mve_sam_decoder_create', ctypes.byref(h), 0, 256, 2, 8, 2048, 4, 256, 3, 2, 64, 1024, f(1e-6), f(1e-5), match='dtype')
    assert not h.value
    bad('mve_sam_decoder_plan', dec._h, 1, 1, 0, 0, None, None, None, match='no prompt')
    bad('mve_sam_decoder_plan', dec._h, 1, 1, 10, 1, None, None, None, match='17 tokens')
    bad('mve_sam_decoder_plan', dec._h, 129, 1, 0, 1, None, None, None, match='at most 128 items')
    bad('mve_sam_decoder_forward', dec._h, p, 1, 1, p, None, None, 0, p, p, None, p, 1 << 20, None, None, match='parameters not loaded', code=-3)
    bad('mve_sam_decoder_finalize', dec._h, None, match='parameters not loaded', code=-3)
    bad('mve_sam_encoder_plan', dec._h, 1, None, None, None, match='a SAM mask decoder, not a SAM image encoder')
    shape = (ctypes.c_longlong * 2)(3, 128)
    bad('mve_unet_load_param', dec._h, b'shared_image_embedding.positional_embedding', p, 0, 2, shape, None, match='expected 256 elements')
    bad('mve_unet_load_param', dec._h, b'prompt_encoder.pe_layer.positional_encoding_gaussian_matrix', p, 0, 2, shape, None, match='not a parameter')


def test_full_size_plan(lib):
    """the ViT-H sized decoder (G = 64): one box, and the largest prompt"""
    from mvedit_amd.sam import SAM_DECODER_CONFIG, TRANSFORMERS_DECODER_CONFIG, SamMaskDecoderEngine
    assert SAM_DECODER_CONFIG['layer_norm_eps'] == 1e-5 and TRANSFORMERS_DECODER_CONFIG['layer_norm_eps'] == 1e-6 and TRANSFORMERS_DECODER_CONFIG['final_layer_norm_eps'] == 1e-5
    eng = SamMaskDecoderEngine(SAM_DECODER_CONFIG, device='cpu')
    one, most = eng.plan(1, 1, 0, True), eng.plan(1, 4, 9, True)
    assert one['n_ops'] == most['n_ops'] == len(eng.op_table()) and one['workspace_bytes'] < most['workspace_bytes'] < 1 << 30
    assert 1e9 < sum(one['flops'].values()) < 1e10
    assert eng.tap_names() == ['tokens', 'queries.0', 'keys.0', 'queries.1', 'keys.1', 'queries.final', 'upscaled', 'hyper_in', 'dense_pe']

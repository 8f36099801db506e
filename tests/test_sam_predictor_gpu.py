"""SamPredictorEngine end to end on the GPU: `set_image` + `predict` over the case-A-sized encoder of the encoder golden's generator and the case-A decoder
of the decoder golden's (image 256, grid 16), equal to running the pieces by hand, and the `sam_predictor` arm of do_segmentation."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, 'golden', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GD, GE = _load('make_sam_decoder_golden'), _load('make_sam_encoder_golden')
_cache = {}


def predictor():
    from mvedit_amd.sam import SamImageEncoderEngine, SamMaskDecoderEngine, SamPredictorEngine
    if 'p' not in _cache:
        f32 = lambda sd: {k: torch.from_numpy(v).float() for k, v in sd.items()}
        enc = SamImageEncoderEngine(GE.config_dict('A'), dtype=torch.float16, device='cuda').load_state_dict(f32(GE.make_weights('A')))
        dec = SamMaskDecoderEngine(GD.config_dict('A'), device='cuda').load_state_dict(f32(GD.make_weights('A')))
        _cache['p'] = SamPredictorEngine(enc, dec, mask_threshold=0.0)
    return _cache['p']


def image(h=150, w=200, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[:h, :w]
    base = 128 + 90 * np.sin(xx / 17.0)[..., None] * np.cos(yy / 11.0)[..., None] * np.array([1.0, 0.6, -0.8])
    return np.clip(base + rs.standard_normal((h, w, 3)) * 12, 0, 255).astype(np.uint8)


BOX = np.array([30, 20, 170, 120])


def test_set_image_and_predict_equal_the_pieces_by_hand():
    from PIL import Image
    from mvedit_amd.sam import postprocess_masks, preprocess_image, preprocess_shape
    p, img = predictor(), image()
    p.set_image(img)
    assert p.is_image_set and p.original_size == (150, 200) and p.input_size == (192, 256) and tuple(p.features.shape) == (1, 256, 16, 16)
    assert p.get_image_embedding() is p.features and p.device.type == 'cuda'
    masks, iou, low = p.predict(box=BOX, multimask_output=True)
    assert masks.shape == (3, 150, 200) and masks.dtype == np.bool_ and iou.shape == (3,) and iou.dtype == np.float32 and low.shape == (3, 64, 64) and low.dtype == np.float32
    assert 0 < masks.sum() < masks.size
    # by hand: host resize -> preprocess -> encoder engine -> decoder engine -> postprocess
    nh, nw = preprocess_shape(150, 200, 256)
    resized = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
    pixels = preprocess_image(torch.from_numpy(resized).cuda(), 256, torch.float16)
    emb = p.encoder.run(pixels)[0]
    assert torch.equal(emb, p.features)
    box = torch.tensor(BOX * np.array([nw / 200, nh / 150, nw / 200, nh / 150]), dtype=torch.float32).reshape(1, 1, 4)
    low2, iou2, _ = p.decoder.run(emb, box, multimask_output=True)
    m2, logits2 = postprocess_masks(low2[0, 0], 256, (nh, nw), (150, 200), 0.0, True)
    assert np.array_equal(low2[0, 0].cpu().numpy(), low) and np.array_equal(iou2[0, 0].cpu().numpy(), iou) and np.array_equal(m2.cpu().numpy(), masks)
    # return_logits: the fp32 logits at (H, W), of which the masks are the sign
    logits, _, _ = p.predict(box=BOX, multimask_output=True, return_logits=True)
    assert logits.dtype == np.float32 and logits.shape == (3, 150, 200) and np.array_equal(logits, logits2.cpu().numpy()) and np.array_equal(logits > 0.0, masks)
    # multimask_output=False: mask token 0 alone
    one, iou1, low1 = p.predict(box=BOX, multimask_output=False)
    assert one.shape == (1, 150, 200) and iou1.shape == (1,) and low1.shape == (1, 64, 64)
    # the same image through set_torch_image
    feats = p.features.clone()
    p.set_torch_image(torch.from_numpy(resized).permute(2, 0, 1)[None].float(), (150, 200))
    assert torch.equal(p.features, feats) and p.input_size == (nh, nw)
    # BGR input is flipped to the model's RGB
    p.set_image(np.ascontiguousarray(img[..., ::-1]), 'BGR')
    assert torch.equal(p.features, feats)


def test_predict_with_points_and_batched_prompts():
    p = predictor()
    p.set_image(image())
    pts, lbl = np.array([[100.0, 70.0], [20.0, 10.0]]), np.array([1, 0])
    m, iou, low = p.predict(point_coords=pts, point_labels=lbl, multimask_output=True)              # padding point: 9 tokens
    mb, ioub, lowb = p.predict(point_coords=pts, point_labels=lbl, box=BOX, multimask_output=True)  # 10 tokens
    assert m.shape == mb.shape == (3, 150, 200) and not np.array_equal(low, lowb)
    sx, sy = 256 / 200, 192 / 150
    boxes = torch.tensor([[30 * sx, 20 * sy, 170 * sx, 120 * sy], [10 * sx, 10 * sy, 90 * sx, 140 * sy]])
    masks, ious, lows = p.predict_torch(boxes=boxes)
    assert masks.shape == (2, 3, 150, 200) and masks.dtype == torch.bool and ious.shape == (2, 3) and lows.shape == (2, 3, 64, 64)
    ref = p.predict(box=BOX)
    assert np.array_equal(masks[0].cpu().numpy(), ref[0]) and np.array_equal(lows[0].cpu().numpy(), ref[2])


def test_do_segmentation_with_the_predictor_engine():
    from mvedit_amd.pipelines.utils import do_segmentation

    class Seg(torch.nn.Module):
        def forward(self, x):
            m = torch.zeros(x.shape[0], 1, *x.shape[2:], device=x.device)
            m[:, :, 20:120, 30:170] = 0.9
            return m
    x = torch.from_numpy(np.stack([image(seed=1), image(seed=2)])).permute(0, 3, 1, 2).float() / 255
    out = do_segmentation(x, Seg(), bg_color=(1.0, 1.0, 1.0), sam_predictor=predictor())
    assert out.shape == (2, 4, 150, 200) and out.dtype == torch.float32 and torch.equal(out[:, :3], x)
    assert set(np.unique(out[:, 3].numpy()).tolist()) <= {0.0, 1.0}
    p = predictor()
    p.set_image((x[1].permute(1, 2, 0) * 255).round().to(torch.uint8).numpy())
    last = p.predict(box=np.array([30, 20, 170, 120]), multimask_output=True)[0][-1]
    img = (x[1].permute(1, 2, 0) * 255).round().numpy()
    near_bg = np.all(img >= 255 - 0.25 * 255, axis=-1)
    assert np.array_equal(out[1, 3].numpy() > 0, last | ~near_bg)

"""Golden for the CLIP text engine: transformers' own `CLIPTextModel` / `CLIPTextModelWithProjection` in float64 on the CPU.

    python tests/golden/make_clip_text_golden.py          (needs `transformers`; writes the two files below)

  tests/golden/clip_text_ref.npz          ids, the float64 outputs the engine is held to (last_hidden_state, hidden_states[-2], pooler_output,
                                          text_embeds), the rel-L2 of transformers' own .half() / .bfloat16() CPU modules against float64 per
                                          output and per hidden state (the engine's bar is 1.5 x these), and the sha256 of every case's weights
  tests/golden/clip_text_hidden_ref.npz   the other entries of hidden_states in float64 (a fault is located by layer)

Two files because one committed file may not exceed 1 MiB.  For the same reason the weights are not stored: `make_weights(case)` below
regenerates them from numpy's frozen `RandomState` stream (bit-stable across numpy versions) and the readers check the sha256 recorded here, so
the values are pinned all the same.  The weights are scaled so that the softmax is not flat and the residual stream reaches a few tens, then
rounded to fp16-representable values: a 16-bit engine that loads them starts from exactly the numbers the float64 reference used (fp16), and
from their one rounding (bf16).

Common geometry: hidden 128, 2 heads, intermediate 512, vocab 512, 77 positions.
  case A   CLIPTextModel, quick_gelu, eos_token_id = 2 (legacy pooling: first position of the maximum id; the end token is the highest id
           and the ids behind it are 0), 2 layers, ids [3, 77] with the end token at positions 5, 20, 76
  case B   CLIPTextModelWithProjection, gelu, eos_token_id = 300 (first-match pooling; ids above 300 occur in front of it, pad 0 behind),
           projection_dim 64, 3 layers, ids [2, 77] (end token at 9 and 50) and a second input [1, 17] (end token at 12)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, 'clip_text_ref.npz')
HIDDEN_REF = os.path.join(HERE, 'clip_text_hidden_ref.npz')

GEOMETRY = dict(vocab_size=512, hidden_size=128, intermediate_size=512, num_attention_heads=2, max_position_embeddings=77, layer_norm_eps=1e-5,
                projection_dim=64, pad_token_id=0, bos_token_id=1)
CASES = {
    'A': dict(with_projection=False, hidden_act='quick_gelu', eos_token_id=2, num_hidden_layers=2, seed=1701, inputs=[dict(B=3, L=77, eos_pos=(5, 20, 76))]),
    'B': dict(with_projection=True, hidden_act='gelu', eos_token_id=300, num_hidden_layers=3, seed=1702,
              inputs=[dict(B=2, L=77, eos_pos=(9, 50)), dict(B=1, L=17, eos_pos=(12,))]),
}
OUTPUTS = ('last_hidden_state', 'penultimate', 'pooler_output', 'text_embeds')


def config_dict(case):
    c = dict(GEOMETRY)
    c.update({k: CASES[case][k] for k in ('hidden_act', 'eos_token_id', 'num_hidden_layers')})
    return c


def _fp16(a):
    return a.astype(np.float16).astype(np.float64)


def make_weights(case):
    """-> {transformers state-dict name: float64 array of fp16-representable values}, from the frozen RandomState stream of the case's seed."""
    cfg, rs = config_dict(case), np.random.RandomState(CASES[case]['seed'])
    C, I, nl = cfg['hidden_size'], cfg['intermediate_size'], cfg['num_hidden_layers']
    sd = {}

    def put(name, shape, std, mean=0.0):
        sd[name] = _fp16(mean + std * rs.standard_normal(shape))

    # transformers' initialisation widths (embeddings 0.02, q/k/v/out hidden^-1/2 (2 layers)^-1/2, fc1 (2 hidden)^-1/2, fc2 as out), linear
    # weights x 4 and embeddings x 10; biases and LayerNorm affine parameters are random too, so that no fused bias path hides behind zeros
    put('text_model.embeddings.token_embedding.weight', (cfg['vocab_size'], C), 0.2)
    put('text_model.embeddings.position_embedding.weight', (cfg['max_position_embeddings'], C), 0.2)
    w_attn, w_fc1 = 4.0 * C ** -0.5 * (2 * nl) ** -0.5, 4.0 * (2 * C) ** -0.5
    for k in range(nl):
        b = f'text_model.encoder.layers.{k}.'
        for n in ('layer_norm1', 'layer_norm2'):
            put(b + n + '.weight', (C,), 0.1, 1.0)
            put(b + n + '.bias', (C,), 0.1)
        for n in ('q_proj', 'k_proj', 'v_proj', 'out_proj'):
            put(b + 'self_attn.' + n + '.weight', (C, C), w_attn)
            put(b + 'self_attn.' + n + '.bias', (C,), 0.1)
        put(b + 'mlp.fc1.weight', (I, C), w_fc1)
        put(b + 'mlp.fc1.bias', (I,), 0.1)
        put(b + 'mlp.fc2.weight', (C, I), w_attn)
        put(b + 'mlp.fc2.bias', (C,), 0.1)
    put('text_model.final_layer_norm.weight', (C,), 0.1, 1.0)
    put('text_model.final_layer_norm.bias', (C,), 0.1)
    if CASES[case]['with_projection']:
        put('text_projection.weight', (cfg['projection_dim'], C), 4.0 * C ** -0.5)
    return sd


def weights_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].astype(np.float16)).tobytes())
    return h.hexdigest()


def make_ids(case, i):
    """int64 [B, L]: random ids in front of the end token, the end token at the listed position, 0 behind it; ids 0 and vocab - 1 both occur."""
    spec, cfg = CASES[case]['inputs'][i], config_dict(case)
    rs = np.random.RandomState(CASES[case]['seed'] * 10 + i)
    V, eos = cfg['vocab_size'], cfg['eos_token_id']
    end = V - 1 if eos == 2 else eos                   # legacy rule: the end token is the highest id
    ids = np.zeros((spec['B'], spec['L']), np.int64)
    for b, p in enumerate(spec['eos_pos']):
        row = rs.randint(1, V - 1 if eos == 2 else V, size=p)
        row[row == end] = 7
        ids[b, :p] = row
        ids[b, p] = end
    if eos != 2:
        ids[0, 1] = V - 1                              # an id above the end token in front of it: the legacy rule would pool this position
    return ids


def build_module(case, dtype):
    import torch
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(**config_dict(case))
    m = (CLIPTextModelWithProjection if CASES[case]['with_projection'] else CLIPTextModel)(cfg)
    sd = {k: torch.from_numpy(v) for k, v in make_weights(case).items()}
    if not hasattr(m, 'text_model'):                   # transformers >= 5: CLIPTextModel holds embeddings / encoder / final_layer_norm itself
        sd = {k[len('text_model.'):]: v for k, v in sd.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def run_module(m, ids, with_projection):
    import torch
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(ids), output_hidden_states=True)
        # CLIPTextModelOutput has no pooler_output: the gathered row is what text_projection consumed
        pooled = m.text_model(input_ids=torch.from_numpy(ids)).pooler_output if with_projection else out.pooler_output
    hs = [h.double().numpy() for h in out.hidden_states]
    res = dict(last_hidden_state=out.last_hidden_state.double().numpy(), penultimate=hs[-2], hidden_states=hs, pooler_output=pooled.double().numpy())
    if with_projection:
        res['text_embeds'] = out.text_embeds.double().numpy()
    return res


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def max_softmax_probability(case, ids, hidden0):
    """Largest attention probability of layer 0 over the rows that see at least 8 keys (row 0 sees one key and has probability 1 by construction)."""
    sd, cfg = make_weights(case), config_dict(case)
    C, H = cfg['hidden_size'], cfg['num_attention_heads']
    b = 'text_model.encoder.layers.0.'
    x = hidden0
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    n = (x - mu) / np.sqrt(var + cfg['layer_norm_eps']) * sd[b + 'layer_norm1.weight'] + sd[b + 'layer_norm1.bias']
    q = n @ sd[b + 'self_attn.q_proj.weight'].T + sd[b + 'self_attn.q_proj.bias']
    k = n @ sd[b + 'self_attn.k_proj.weight'].T + sd[b + 'self_attn.k_proj.bias']
    B, L, _ = x.shape
    q, k = q.reshape(B, L, H, C // H).transpose(0, 2, 1, 3), k.reshape(B, L, H, C // H).transpose(0, 2, 1, 3)
    s = q @ k.transpose(0, 1, 3, 2) * (C // H) ** -0.5
    s = np.where(np.tril(np.ones((L, L), bool)), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return float(p[:, :, 8:, :].max()) if L > 8 else float('nan')


def generate(case):
    """-> (headline dict, hidden dict) of arrays for one case."""
    import torch
    wp = CASES[case]['with_projection']
    head, hidden = {}, {}
    head[f'{case}.weights_sha256'] = np.array(weights_digest(make_weights(case)))
    m64 = build_module(case, torch.float64)
    lows = {'fp16': build_module(case, torch.float16), 'bf16': build_module(case, torch.bfloat16)}
    for i, spec in enumerate(CASES[case]['inputs']):
        ids = make_ids(case, i)
        ref = run_module(m64, ids, wp)
        key = f'{case}.{i}.'
        head[key + 'ids'] = ids
        for b, p in enumerate(spec['eos_pos']):
            assert np.array_equal(ref['pooler_output'][b], ref['last_hidden_state'][b, p]), (case, i, b, 'pooler_output is not the row at the intended position')
        pmax = max_softmax_probability(case, ids, ref['hidden_states'][0])
        assert pmax > 0.5, (case, i, pmax, 'the softmax is too flat to tell a wrong mask')
        head[key + 'max_softmax_probability'] = np.array(pmax)
        head[key + 'penultimate_absmax'] = np.array(np.abs(ref['penultimate']).max())
        for o in OUTPUTS:
            if o in ref:
                head[key + o] = ref[o]
        for k, h in enumerate(ref['hidden_states']):
            if k != len(ref['hidden_states']) - 2:     # hidden_states[-2] is `penultimate` of the first file
                hidden[key + f'hidden_states.{k}'] = h
        for tag, m in lows.items():
            low = run_module(m, ids, wp)
            for o in OUTPUTS:
                if o in ref:
                    err = rel_l2(low[o], ref[o])
                    head[key + f'err_{tag}.' + o] = np.array(err)
                    if tag == 'fp16':
                        assert err < 5e-3, (case, i, o, err, 'the fixture is too hot to discriminate')
            head[key + f'err_{tag}.hidden_states'] = np.array([rel_l2(a, b) for a, b in zip(low['hidden_states'], ref['hidden_states'])])
    return head, hidden


def main():
    head, hidden = {}, {}
    for case in CASES:
        h, hh = generate(case)
        head.update(h)
        hidden.update(hh)
    np.savez_compressed(REF, **head)
    np.savez_compressed(HIDDEN_REF, **hidden)
    for k in sorted(head):
        if head[k].ndim == 0:
            print(f'{k:44s} {head[k]}')
    for p in (REF, HIDDEN_REF):
        print(p, os.path.getsize(p), 'bytes')
        assert os.path.getsize(p) < (1 << 20), 'a committed file may not exceed 1 MiB'


if __name__ == '__main__':
    sys.exit(main())

"""What the transformer surrogate families share on the Python side: the methods every spec repeats (`TokenSpec`), the record a
family's block of `graphs.py` ends with (`Family`: one row of `graphs.FAMILIES`), and the pieces its synthetic-weight rules are made of.

A family's block of `graphs.py` holds everything Python knows about the family: its `*_MODELS` table, its `*Spec`, `is_*_name` /
`*_named` / the test-size twins, its synthetic draw rules, its checkpoint checks and key aliases, the values of its ctypes config, and
the command line's words for it."""
from types import MappingProxyType
from typing import Callable, Dict, Mapping, NamedTuple, Optional, Sequence


class TokenSpec:
    """Methods only (no fields: every spec keeps its positional construction).  A spec of a flat family (`blocks` blocks of one width)
    has `tokens` and `dim` as values; a staged one derives from `StagedSpec`."""
    #: arguments of the create entry between the config and the weight pointers (ViT's prefix count, for `i2v_vit_create_ex`)
    create_extra = ()

    @property
    def in_hw(self):
        return (self.img, self.img)

    def hook_for(self, depth: int, whole_module: bool = False) -> int:
        """Zero-based block / stage whose output depth `depth` hooks (`whole_module` changes nothing: a block is one module)."""
        if depth not in self.hooks:
            raise KeyError(depth)
        return self.hooks[depth]

    def quarter_hooks(self) -> Dict[int, int]:
        """Depth d (1..4) -> zero-based block d * blocks / 4 - 1: the last block of every quarter of the stack."""
        return {d: d * self.blocks // 4 - 1 for d in (1, 2, 3, 4)}

    def hook_shape(self, where: int):
        """(tokens, width) of the stream hooked behind block / stage `where`."""
        return (self.tokens, self.dim)

    @property
    def units(self) -> int:
        """How many blocks / stages the create entry counts hooks and weights in."""
        return self.blocks

    def config_values(self) -> Sequence:
        """The fields of the family's `lib.*Config` in the struct's order: ints, floats, and sequences for the array fields (the engine
        pads a sequence with zeros to the array's length)."""
        raise NotImplementedError


class StagedSpec(TokenSpec):
    """A pyramid: hooks and weights count stages, and `tokens(i)` / `width(i)` are per stage."""

    def hook_shape(self, where: int):
        return (self.tokens(where), self.width(where))

    @property
    def units(self) -> int:
        return self.stages


class Family(NamedTuple):
    """One row of `graphs.FAMILIES`."""
    word: str                       # the word in the C entries (`i2v_<word>_*`) and in `lib.FAMILY_PROTOS`
    spec: type                      # the spec class
    models: Dict[str, tuple]        # the served names
    is_name: Callable               # name -> bool: a name of the family's vocabulary, served or not
    named: Callable                 # (name, in_hw) -> spec, or the refusal
    tiny_twin: Callable             # (served name, in_hw) -> the test-size twin that stands for it
    help: str                       # the command line's phrase in front of the served names
    hooked: str                     # ... and the depth error's phrase for what `hooks` numbers ("blocks {}")
    in_build: bool                  # `graphs.build` knows the family (else `build_surrogate` alone does)
    synthetic: Sequence             # (key matcher, draw) rules of the synthetic weights: the first match wins
    check: Optional[Callable] = None            # (spec, state dict, where) -> None, or the refusal of a checkpoint of another model
    key_aliases: Mapping[str, str] = MappingProxyType({})       # checkpoint key -> the key `param_shapes()` knows it by


# ---------------------------------------------------------------------------
# synthetic weights: key matchers and draws.  A draw is (shape, generator) -> tensor; `weights.synthetic_state_dict` gives every key
# a generator of its own, so a draw's values depend on the key and the seed alone.
# ---------------------------------------------------------------------------
def ends(*suffixes):
    return lambda k: k.endswith(suffixes)


def starts(*prefixes):
    return lambda k: k.startswith(prefixes)


def keys(*names):
    return lambda k: k in names


def always(k):
    return True


def _randn(shp, g):
    import torch            # (inside the draws, as everywhere in `graphs`: importing the architectures does not import torch)
    return torch.randn(*shp, generator=g)


def _rand(shp, g):
    import torch
    return torch.rand(*shp, generator=g)


def _sign(shp, g):
    import torch
    return torch.randint(0, 2, shp, generator=g).float() * 2 - 1


def normal(std=1.0):
    return lambda shp, g: std * _randn(shp, g)


def normal_over(div):
    return lambda shp, g: _randn(shp, g) / div


def uniform(low, span=1.0):
    return lambda shp, g: low + span * _rand(shp, g)


def signed_uniform(low, span):
    """Uniform on (low, low + span) with a random sign."""
    return lambda shp, g: (low + span * _rand(shp, g)) * _sign(shp, g)


def clamped(std):
    """Truncated-normal-like, as timm initialises matrices: N(0, 1) clamped at 2, times `std`."""
    return lambda shp, g: _randn(shp, g).clamp_(-2.0, 2.0) * std


def fan_in(factor=1.0):
    """`factor` fan_in^-0.5 N(0, 1): a unit-variance input gives an output of variance factor^2."""
    def draw(shp, g):
        n = 1
        for v in shp[1:]:
            n *= v
        return _randn(shp, g) * (factor * n ** -0.5)
    return draw


def norm_gain(shp, g):
    """A LayerNorm gain: 1 + 0.1 N(0, 1)."""
    return 1.0 + 0.1 * _randn(shp, g)


SMALL_BIAS = normal(0.02)


def fan_in_tail(norms, half=ends("fc2.weight", "attn.proj.weight"), bias=ends("bias")):
    """The tail ten families share behind their own rules: LayerNorm gains 1 + 0.1 N(0, 1) (`norms` matches them), biases 0.02 N(0, 1),
    and every other array -- the Linears and convolutions -- fan_in^-0.5 N(0, 1), which keeps a unit-variance stream and puts the
    attention logits at O(1); the arrays `half` matches (the second Linear of every residual branch) at half that, so that each
    block adds a few tenths to its stream."""
    return [(norms, norm_gain), (bias, SMALL_BIAS), (half, fan_in(0.5)), (always, fan_in(1.0))]


def clamped_tail(norms, qkv_draw):
    """ViT's and Swin's tail: LayerNorm gains near 1, small biases, `attn.qkv.weight` by `qkv_draw`, every other matrix at std 0.02
    clamped at 2 std, as timm initialises them."""
    return [(norms, norm_gain), (ends("bias"), SMALL_BIAS), (ends("attn.qkv.weight"), qkv_draw), (always, clamped(0.02))]

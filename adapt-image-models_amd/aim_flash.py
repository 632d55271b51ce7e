"""``AIM_FLASH`` backbone: ``AIM_FLASH_WIN`` whose odd blocks run their window attention on windows shifted by half a window.

Drop-in for ``mmaction/models/backbones/vitclip_aim_flash.py:402-560`` of the reference at ``wind_attn=True, win_prompt=False``
(what its three recipes, ``configs/recognition/vit/AIM/AIM_flash_base_{hmdb51,diving48,ucf101}.py``, use): same registry
name, constructor keywords, parameter names and shapes, freeze policy, ``init_weights`` and DropPath draws as ``AIM_FLASH_WIN``
(aim_flash_win.py; the two reference files differ in the block's forward alone).

The shifted block (reference ``:217-298``) rolls the [T, G, G] grid by minus the shift, cuts the rolled grid's last window
along h and along w into the strips ``[-w:-s]`` and ``[-s:]``, runs attention inside every piece and stitches the pieces back
with nine ``cat``s and a second roll.  In the ORIGINAL coordinates that is a partition of the grid into boxes: the h and w
axes are cut at 0, s, s + w, s + 2 w, ... (nothing wraps: the rolled strips are the axis' last and first segment), the t axis
keeps whole windows that start at st and wrap round the clip's end.  ``aim_win_attn_fwd_shift`` / ``aim_win_attn_bwd_shift``
take that rule as addresses, so the block is ``aim_flash_win._block_forward`` with one more argument (which goes to
``win_block.win_temporal_forward``, where steps 1-3 live) and no rolled,
strip-ordered or stitched copy of anything exists.

Block i is shifted when ``i % 2 == 1 and not not_shift``, by ``window_size[k] // 2``, zeroed on every axis where the grid does
not exceed the window (the reference's ``get_window_size``); if all three come out 0 no block is shifted.  The reference
cannot run a geometry in which some shift is non-zero while the h or the w shift is 0 (an empty strip: ``ZeroDivisionError`` /
``EinopsError``); the constructor refuses it.
"""
from .aim_flash_win import AIM_FLASH_WIN
from .registry import BACKBONES
from .win_block import clip_shift


def check_shift(shift, window_size, T: int, G: int):
    st, sh, sw = shift
    if (st or sh or sw) and (sh == 0 or sw == 0):
        raise ValueError(f"window_size={tuple(window_size)} on the {T} x {G} x {G} grid gives the shift {(st, sh, sw)}: the "
                         "reference cannot run a shifted block whose h or w shift is 0 (its border strip is empty)")


@BACKBONES.register_module()
class AIM_FLASH(AIM_FLASH_WIN):
    """AIM with shifted 3-D window temporal attention in every odd block (reference vitclip_aim_flash.py:402-560)."""

    def __init__(self, input_resolution: int, num_frames: int, patch_size: int, width: int, layers: int, heads: int,
                 drop_path_rate, num_tadapter=1, adapter_scale=0.5, pretrained=None, checkpoint=False, use_flash_attn=True,
                 prompt=True, wind_attn=False, window_size=(32, 2, 2), not_shift=True, win_prompt=False):
        if win_prompt:
            raise NotImplementedError("AIM_FLASH(win_prompt=True) (vitclip_aim_flash.py:269-286: the class tokens of a window's "
                                      "frames as prompts of the window) is not built; no recipe uses it")
        super().__init__(input_resolution, num_frames, patch_size, width, layers, heads, drop_path_rate,
                         num_tadapter=num_tadapter, adapter_scale=adapter_scale, pretrained=pretrained, checkpoint=checkpoint,
                         use_flash_attn=use_flash_attn, prompt=prompt, wind_attn=wind_attn, window_size=window_size,
                         not_shift=True)
        self.not_shift, self.win_prompt = bool(not_shift), win_prompt
        self.variant = 'aim_flash'
        if not self.not_shift:
            G = input_resolution // patch_size
            check_shift(clip_shift(self.window_size, num_frames, G), self.window_size, num_frames, G)

    def _block_shift(self, i: int, T: int, G: int):
        if self.not_shift or i % 2 == 0:
            return None
        shift = clip_shift(self.window_size, T, G)
        if not any(shift):
            return None
        check_shift(shift, self.window_size, T, G)
        return shift

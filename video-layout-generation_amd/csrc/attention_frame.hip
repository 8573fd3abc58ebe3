// Frame-local attention (option attention = "factored", its odd layers): vlg_attention_frame_fwd / _bwd / _step and their
// bf16 forms.  The kernels are the templates of attention_clip.hip instantiated with FRAME = true - rules, tile ranges and
// classification are described there; this unit only keeps those instantiations out of the block-causal code objects.
#define VLG_ATTENTION_FRAME_TU 1
#include "attention_clip.hip"

// Dense self-attention for SHORT sequences with any head_dim <= 128 (include/lkgd_hip.h section 16): the attention of the
// CLIP-ViT-H image encoder in front of the loop (257 tokens, 16 heads of 80 channels - the head_dim-64 flash kernel does not
// fit; /root/reference/pipeline/pipeline_stable_video_diffusion_trans.py:164-203 runs `self.image_encoder(image).image_embeds`
// once per clip).  10.8 GFLOP per encoded image in 32 launches: a boundary stage, written for exactness and brevity, not for the
// matrix pipe - fp16 operands, every product and sum in fp32.  The kernel, its checks and its launch: attn_dense.h.
#include "attn_dense.h"

extern "C" int lkgd_attn_dense(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* out,
                               int32_t ldo, int32_t nbatch, int32_t S, int32_t heads, int32_t head_dim, float scale,
                               lkgd_stream_t stream) {
  return attn_dense_launch<false>(q, ldq, k, ldk, v, ldv, out, ldo, nbatch, S, heads, head_dim, nullptr, scale, stream);
}

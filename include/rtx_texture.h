/* Replacing the texture maps and the skybox of a live scene from device memory.  An extension of the C ABI in rtx.h --
 * the reference has no such call; a new texture there means a new image file and loading the scene file again, and a scene edited here
 * renders, bit for bit, what a scene created from a description holding the new maps renders.
 *
 * Ordering and errors follow rtx_scene_edit.h: rtx_scene_set_map and rtx_scene_set_sky wait for everything queued on the scene and for
 * `stream`, where the caller produced the texels; renders queued before them see the old scene, renders queued after them the new one, and
 * the caller's buffers may be reused once the call returns.  A refused argument (RTX_ERR_ARG) leaves the scene as it was.
 * rtx_scene_write_texels alone is asynchronous: see there. */
#ifndef RTX_TEXTURE_H
#define RTX_TEXTURE_H
#include "rtx.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { RTX_TEX_DIFFUSE = 0, RTX_TEX_NORMAL = 1, RTX_TEX_SPECULAR = 2, RTX_TEX_SKY = 3 };
enum { RTX_TEXELS_STORED = 0,   /* fp32 exactly as the scene stores them: 3 per texel, 1 for SPECULAR; copied verbatim */
       RTX_TEXELS_RGB8   = 1 }; /* 3 bytes per texel, R G B = what loadBMP returns; decoded with the loader's arithmetic of `kind`:
                                   c = byte / 256; DIFFUSE and SKY keep c, NORMAL keeps Vec3f(c.x*2-1, -(c.y*2-1), c.z).normalize(),
                                   SPECULAR keeps (c.x+c.y+c.z)/3.0f */

typedef struct rtx_texels {
	int32_t format;          /* RTX_TEXELS_* */
	uint32_t width, height;
	const void* data_dev;    /* first texel of row 0, device memory (STORED: 4-byte aligned) */
	int64_t row_pitch;       /* bytes from row r to row r+1; may be negative (a top-down image handed in from its last row);
	                            |row_pitch| >= one row (STORED: a multiple of 4) */
} rtx_texels;

/* Row 0 is the first STORED row: the bottom row of a BMP, since the loader keeps file order. */

/* Replace map `kind` (RTX_TEX_DIFFUSE / NORMAL / SPECULAR) of mesh `mesh` as a whole: the size may change, a map may appear where the mesh
 * had none, texels == NULL removes the map.  Afterwards the device holds what rtx_scene_create would have uploaded for a description with
 * this map: the mesh's record carries the new pointer and size, the old allocation is freed (rtx_scene_bytes reports a fresh scene's
 * number); the mesh's geometry, tree, uv and prune copies are not touched.  Refused: a bad mesh index, kind or format, RTX_TEX_SKY, a zero
 * width or height, data_dev == NULL, |row_pitch| below one row, a normal map for a mesh without tangents on the device.  The new map is
 * allocated before the old one is dropped: a failed allocation leaves the old map in place. */
int rtx_scene_set_map(rtx_scene* scene, uint32_t mesh, int32_t kind, const rtx_texels* texels, void* stream);

/* The same for the six skybox faces, which share one size and one format.  A scene without a skybox gains one (the view's
 * RTX_FLAG_SKYBOX may then be set); faces == NULL: the scene loses its skybox, refused while the current view has that flag set. */
int rtx_scene_set_sky(rtx_scene* scene, const rtx_texels faces[6], void* stream);

/* Write a rectangle of texels at (x0, y0) into a map (index: the mesh) or a sky face (index: 0..5) that exists; the rectangle must lie
 * inside it, texels outside it keep their bits.  Asynchronous on `stream`: no allocation, no host wait, nothing on the NULL stream.
 * Renders queued on that stream before the call see the old texels, later ones the new; ordering against renders on other streams is the
 * caller's job, as for a framebuffer, and `texels` must stay as it is until the stream has passed the call. */
int rtx_scene_write_texels(rtx_scene* scene, int32_t kind, uint32_t index, uint32_t x0, uint32_t y0, const rtx_texels* texels, void* stream);

/* Size and device pointer of a map or sky face as it is now (0, 0, NULL where there is none). */
int rtx_scene_texture_info(rtx_scene* scene, int32_t kind, uint32_t index, uint32_t* width, uint32_t* height, const float** texels_dev);

#ifdef __cplusplus
}
#endif
#endif

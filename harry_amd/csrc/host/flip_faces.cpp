// hry_mesh_flip_faces: a mesh with some of its faces turned round (include/harry_amd.h; the flags usually come from
// hry_orient_build's "face_flip").  The first corner of a face stays where it is: (v0, v1, ..., vk-1) becomes (v0, vk-1, ..., v1), so
// a triangle of the fan (v0, vi, vi+1) reads (v0, vi+1, vi) afterwards.
#include <memory>

#include "host.hpp"

namespace hry {

Mesh *mesh_flip_faces(const Mesh &m, const uint32_t *face_flip)
{
	if (m.partial) throw Error(HRY_E_ARG, "flip faces: a partial mesh");
	std::unique_ptr<Mesh> c(new Mesh(m));
	c->device_token = 0; c->render_token = 0; c->order_token = 0;
	const int nb = m.general ? m.bind.nb_corner : 0;
	const bool rows = nb > 0 && m.bind.corner_attr.size() == (size_t)m.ne() * nb;
	for (uint32_t f = 0; f < m.nf; ++f) {
		if (!face_flip[f]) continue;
		const uint32_t b = m.face_off[f], k = m.face_off[f + 1] - b;
		for (uint32_t j = 1; j < k; ++j) {   // corner j comes from corner k - j
			c->org[b + j] = m.org[b + k - j];
			if (rows) for (int a = 0; a < nb; ++a) c->bind.corner_attr[(size_t)(b + j) * nb + a] = m.bind.corner_attr[(size_t)(b + k - j) * nb + a];
		}
	}
	c->twin.clear();   // matched afresh, on the device at the first upload or by ensure_twins
	c->twins_pending = true;
	return c.release();
}

}   // namespace hry

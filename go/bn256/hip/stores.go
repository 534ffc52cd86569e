package hip

/*
#include <stdlib.h>
#include "handel_gpu.h"
*/
import "C"

import (
	"unsafe"
)

// Stores is the device-resident scoring state of the Handel instances one
// process hosts (hg_stores_*): per receiver and level the best bitset, whether
// there is one, and the verified individual signatures (store.go:39-80). The
// host store stays authoritative: Store / unsafeCheckMerge (store.go:82-226)
// run on the host once per verified signature and the changed levels are
// pushed with Update; only Evaluate (store.go:101-183), which runs once per
// queued signature per step, runs on the device. That is the default; after
// EnableMerge the signatures are resident too and MergeDevice / Combined run
// the rest of the store on the device (see below).
//
// A Stores belongs to the registry its engine held when it was made: after a
// later LoadRegistry every call fails. Close it before its engine.
type Stores struct {
	e      *Engine
	h      *C.hg_stores
	stride int
}

// StoreUpdate is the new state of one (receiver, level): Best nil means the
// level has no best multisignature. Both bitsets are willf words of the
// level's size (bit i = word[i>>6] bit i&63).
type StoreUpdate struct {
	Receiver, Level int
	Best            []uint64
	Individuals     []uint64
}

// NewStores creates the stores of the hosted receivers (distinct registry
// indices); maxPackets sizes the workspaces of Evaluate and SelectDevice.
func (e *Engine) NewStores(receivers []int, maxPackets int) (*Stores, error) {
	ids := make([]C.uint32_t, len(receivers))
	for i, r := range receivers {
		ids[i] = C.uint32_t(r)
	}
	var p *C.uint32_t
	if len(ids) > 0 {
		p = &ids[0]
	}
	var h *C.hg_stores
	rc := C.hg_stores_create(e.ctx, p, C.size_t(len(ids)), C.size_t(maxPackets), &h)
	if rc != C.HG_OK {
		return nil, e.fail(rc)
	}
	return &Stores{e: e, h: h, stride: int(C.hg_packet_stride_words(e.ctx))}, nil
}

// Close releases the device tables.
func (s *Stores) Close() {
	if s.h != nil {
		C.hg_stores_destroy(s.h)
		s.h = nil
	}
}

// Update replaces the state of the named (receiver, level) pairs, each named
// at most once: one host-to-device copy and one scatter kernel. Call it after
// the host store's Store calls of a step with the levels they changed.
func (s *Stores) Update(ups []StoreUpdate) error {
	if len(ups) == 0 {
		return nil
	}
	recs := make([]C.hg_store_update, len(ups))
	var words []uint64
	for i, u := range ups {
		recs[i] = C.hg_store_update{receiver: C.uint32_t(u.Receiver), level: C.uint32_t(u.Level)}
		if u.Best != nil {
			recs[i].flags = C.HG_STORE_HAS_BEST
			recs[i].best_off = C.uint32_t(len(words))
			words = append(words, u.Best...)
		}
		recs[i].indiv_off = C.uint32_t(len(words))
		words = append(words, u.Individuals...)
	}
	rc := C.hg_stores_update(s.h, &recs[0], C.size_t(len(recs)), wordPtr(words), C.size_t(len(words)))
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// Read returns one level's device state: the best bitset's words, the
// verified individual signatures' words, and whether the level has a best.
func (s *Stores) Read(receiver, level int) (best, individuals []uint64, hasBest bool, err error) {
	best = make([]uint64, s.stride)
	individuals = make([]uint64, s.stride)
	var has C.int
	rc := C.hg_stores_read(s.h, C.uint32_t(receiver), C.uint32_t(level), wordPtr(best), wordPtr(individuals), &has)
	if rc != C.HG_OK {
		return nil, nil, false, s.e.fail(rc)
	}
	return best, individuals, has != 0, nil
}

// Evaluate scores the 2n slots a ParsePackets-shaped parse wrote (slot i:
// packet i's multisignature, slot n+i: its individual signature; a slot's
// words at slot*stride): store.go:111-183 against each receiver's store at the
// packet's level. live (nil, or 2n bytes) is the caller's
// IndividualSigFilter / rcvCompleted mask. Scores: 0 for a slot whose code is
// not HG_OK, that is not live, or whose (receiver, level) has no range; -1 for
// a receiver without a store; else the reference's mark.
func (s *Stores) Evaluate(recs []C.hg_packet, stride int, words []uint64, codes []int32, live []byte) ([]int32, error) {
	n := len(recs)
	if n == 0 {
		return nil, nil
	}
	if len(words) != 2*n*stride || len(codes) != 2*n || (live != nil && len(live) != 2*n) {
		return nil, &DeviceError{Code: C.HG_ERR_ARG, Msg: "Evaluate: words, codes and live must cover 2n slots"}
	}
	scores := make([]int32, 2*n)
	rc := C.hg_stores_evaluate(s.h, &recs[0], C.size_t(n), C.size_t(stride), wordPtr(words), codePtr(codes),
		bytePtr(live), codePtr(scores))
	if rc != C.HG_OK {
		return nil, s.e.fail(rc)
	}
	return scores, nil
}

// EvaluateDevice is Evaluate on arrays already in device memory (the outputs
// of hg_parse_packets_device), asynchronous on stream (nil: the engine's).
func (s *Stores) EvaluateDevice(dPkts unsafe.Pointer, n, stride int, dWords, dCodes, dLive, dScores,
	stream unsafe.Pointer) error {
	rc := C.hg_stores_evaluate_device(s.h, (*C.hg_packet)(dPkts), C.size_t(n), C.size_t(stride),
		(*C.uint64_t)(dWords), (*C.int32_t)(dCodes), (*C.uint8_t)(dLive), (*C.int32_t)(dScores), stream)
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// SelectCapacity is the number of entries SelectDevice writes for n packets
// and k picks per store: min(2n, stores*k).
func (s *Stores) SelectCapacity(n, k int) int {
	return int(C.hg_stores_select_capacity(s.h, C.size_t(n), C.uint32_t(k)))
}

// SelectDevice is readTodos with k slots per store (processing.go:171-220) on
// device arrays: the k best slots of score > 0 per store (ties: a packet's
// multisignature before its individual signature, earlier packets first),
// grouped by store, with their requests and signatures gathered into
// dOutReqs / dOutSigs for hg_verify_aggregate_device. Entries from *dCount to
// SelectCapacity hold a request that fails the level check, so the whole
// capacity may be verified without reading the count back.
func (s *Stores) SelectDevice(dPkts unsafe.Pointer, n int, dScores unsafe.Pointer, k int, dReqs, dSigs, dSel, dCount,
	dOutReqs, dOutSigs, stream unsafe.Pointer) error {
	rc := C.hg_stores_select_device(s.h, (*C.hg_packet)(dPkts), C.size_t(n), (*C.int32_t)(dScores), C.uint32_t(k),
		(*C.hg_request)(dReqs), (*C.uint8_t)(dSigs), (*C.uint32_t)(dSel), (*C.uint32_t)(dCount),
		(*C.hg_request)(dOutReqs), (*C.uint8_t)(dOutSigs), stream)
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// StoreSig is one signature loaded into a merge-enabled Stores: Level 0 is the
// receiver's own signature (Index ignored); Index = BestSig loads the level's
// best signature, any other Index the individual signature at that mapped
// index of the level. Sig is the 64-byte marshal.
type StoreSig struct {
	Receiver, Level int
	Index           uint32
	Sig             []byte
}

// BestSig is StoreSig.Index for a level's best signature; FullLevel is
// StoreQuery.Level for FullSignature.
const (
	BestSig   = uint32(C.HG_STORE_SIG_BEST)
	FullLevel = uint32(C.HG_STORE_LEVEL_FULL)
)

// StoreQuery names one Combined(level) (store.go:248-262), or, with Level =
// FullLevel, one FullSignature (store.go:238-246).
type StoreQuery struct {
	Receiver int
	Level    uint32
}

// Combined is one outgoing multisignature: Code is HG_OK, HG_COMBINED_EMPTY
// (the reference returns nil), HG_COMBINED_ERR_MISSING or HG_ERR_ARG.
type Combined struct {
	Code      int32
	BitLength int
	Words     []uint64
	Sig       []byte
}

// EnableMerge makes the store complete on the device: the best signatures, the
// own signature and the verified individual signatures become resident, and
// MergeDevice / Combined replace the host store's Store / unsafeCheckMerge
// (store.go:82-229) and Combined / FullSignature. Opt-in: a Stores that never
// calls it behaves as before.
func (s *Stores) EnableMerge() error {
	if rc := C.hg_stores_enable_merge(s.h); rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// UpdateSigs loads signatures from the host (seeding, and a host store's
// mirror), each target named at most once. Call it after Update: Update clears
// a level's "best signature known" bit.
func (s *Stores) UpdateSigs(sigs []StoreSig) error {
	if len(sigs) == 0 {
		return nil
	}
	recs := make([]C.hg_store_sig, len(sigs))
	buf := make([]byte, 0, 64*len(sigs))
	for i, g := range sigs {
		if len(g.Sig) != 64 {
			return &DeviceError{Code: C.HG_ERR_ARG, Msg: "UpdateSigs: a signature marshal is 64 bytes"}
		}
		recs[i] = C.hg_store_sig{receiver: C.uint32_t(g.Receiver), level: C.uint32_t(g.Level),
			index: C.uint32_t(g.Index), sig_off: C.uint32_t(i)}
		buf = append(buf, g.Sig...)
	}
	rc := C.hg_stores_update_sigs(s.h, &recs[0], C.size_t(len(recs)), bytePtr(buf), C.size_t(len(sigs)))
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// ReadBest returns one level's best (store.go:231-236 Best): its bitset's
// words, its signature, whether there is one and whether its signature is
// held. Level 0 is the own signature.
func (s *Stores) ReadBest(receiver, level int) (best []uint64, sig []byte, hasBest, sigKnown bool, err error) {
	best = make([]uint64, s.stride)
	sig = make([]byte, 64)
	var flags C.int
	rc := C.hg_stores_read_best(s.h, C.uint32_t(receiver), C.uint32_t(level), wordPtr(best), bytePtr(sig), &flags)
	if rc != C.HG_OK {
		return nil, nil, false, false, s.e.fail(rc)
	}
	return best, sig, flags&C.HG_STORE_HAS_BEST != 0, flags&C.HG_STORE_BEST_SIG != 0, nil
}

// MergeDevice is store.go:82-99 Store for the picks of one intake step, on
// device arrays and asynchronous on stream: dSel / dCount are SelectDevice's
// output, dVcodes the verdicts of hg_verify_aggregate_device over the same
// capacity, dPkts / dWords / dSigs the parse outputs. dResults receives one
// HG_MERGE_* per entry, dChanged / dNChanged the (receiver, level) pairs whose
// best changed.
func (s *Stores) MergeDevice(dPkts unsafe.Pointer, n int, dSel, dCount unsafe.Pointer, capacity int,
	dVcodes unsafe.Pointer, stride int, dWords, dSigs, dResults, dChanged, dNChanged, stream unsafe.Pointer) error {
	rc := C.hg_stores_merge_device(s.h, (*C.hg_packet)(dPkts), C.size_t(n), (*C.uint32_t)(dSel),
		(*C.uint32_t)(dCount), C.size_t(capacity), (*C.int32_t)(dVcodes), C.size_t(stride), (*C.uint64_t)(dWords),
		(*C.uint8_t)(dSigs), (*C.int32_t)(dResults), (*C.uint32_t)(dChanged), (*C.uint32_t)(dNChanged), stream)
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// Combined answers the queries with the multisignatures Handel sends: the
// bests of levels <= Level in the range the peers of Level+1 expect, or the
// full signature. wordsStride words per result (at least ceil(N/64) when a
// full query is among them).
func (s *Stores) Combined(queries []StoreQuery, wordsStride int) ([]Combined, error) {
	m := len(queries)
	if m == 0 {
		return nil, nil
	}
	qs := make([]C.hg_store_query, m)
	for i, q := range queries {
		qs[i] = C.hg_store_query{receiver: C.uint32_t(q.Receiver), level: C.uint32_t(q.Level)}
	}
	codes := failedCodes(m)
	bitlens := make([]uint32, m)
	words := make([]uint64, m*wordsStride)
	sigs := make([]byte, 64*m)
	rc := C.hg_stores_combined(s.h, &qs[0], C.size_t(m), C.size_t(wordsStride), codePtr(codes),
		(*C.uint32_t)(unsafe.Pointer(&bitlens[0])), wordPtr(words), bytePtr(sigs))
	if rc != C.HG_OK {
		return nil, s.e.fail(rc)
	}
	out := make([]Combined, m)
	for i := range out {
		out[i] = Combined{Code: codes[i], BitLength: int(bitlens[i]),
			Words: words[i*wordsStride : (i+1)*wordsStride], Sig: sigs[64*i : 64*i+64]}
	}
	return out, nil
}

// CombinedDevice is Combined on device arrays, asynchronous on stream.
func (s *Stores) CombinedDevice(dQueries unsafe.Pointer, m, wordsStride int, dCodes, dBitlens, dWords, dSigs,
	stream unsafe.Pointer) error {
	rc := C.hg_stores_combined_device(s.h, (*C.hg_store_query)(dQueries), C.size_t(m), C.size_t(wordsStride),
		(*C.int32_t)(dCodes), (*C.uint32_t)(dBitlens), (*C.uint64_t)(dWords), (*C.uint8_t)(dSigs), stream)
	if rc != C.HG_OK {
		return s.e.fail(rc)
	}
	return nil
}

// Pool is Handel's queue of parsed signatures kept in device memory across
// intake steps (hg_stores_pool_*): AppendDevice adds the admitted slots of a
// parsed batch, StepDevice is one readTodos pass (processing.go:171-220) over
// the whole queue whose picks come out as a parsed batch for
// hg_verify_aggregate_device and MergeDevice, the rest staying queued in
// readTodos' order. Close it before its Stores.
type Pool struct {
	s *Stores
	h *C.hg_pool
}

// PooledSlot is one queued slot as Read returns it.
type PooledSlot struct {
	Origin, Receiver, Level int
	Individual              bool
	Mark                    int32 // of the last step; 0 for a slot appended since
}

// NewPool allocates a pool of capacitySlots slots, workspaces included; no
// later call allocates device memory.
func (s *Stores) NewPool(capacitySlots int) (*Pool, error) {
	var h *C.hg_pool
	rc := C.hg_stores_pool_create(s.h, C.size_t(capacitySlots), &h)
	if rc != C.HG_OK {
		return nil, s.e.fail(rc)
	}
	return &Pool{s: s, h: h}, nil
}

// Close releases the pool's device memory.
func (p *Pool) Close() {
	if p.h != nil {
		C.hg_stores_pool_destroy(p.h)
		p.h = nil
	}
}

// Bytes is the device memory the pool holds.
func (p *Pool) Bytes() int { return int(C.hg_stores_pool_bytes(p.h)) }

// AppendDevice queues the admitted slots of one hg_parse_packets_device call
// (its inputs dPkts, n, stride and its outputs; dLive nil or the caller's 2n
// mask), in Handel's queue order, asynchronous on stream. It fails without
// appending when 2n slots do not fit.
func (p *Pool) AppendDevice(dPkts unsafe.Pointer, n, stride int, dReqs, dWords, dSigs, dCodes, dLive,
	stream unsafe.Pointer) error {
	rc := C.hg_stores_pool_append_device(p.h, (*C.hg_packet)(dPkts), C.size_t(n), C.size_t(stride),
		(*C.hg_request)(dReqs), (*C.uint64_t)(dWords), (*C.uint8_t)(dSigs), (*C.int32_t)(dCodes),
		(*C.uint8_t)(dLive), stream)
	if rc != C.HG_OK {
		return p.s.e.fail(rc)
	}
	return nil
}

// SelectCapacity is the number of entries StepDevice writes for k slots per
// store.
func (p *Pool) SelectCapacity(k int) int {
	return int(C.hg_stores_pool_select_capacity(p.h, C.uint32_t(k)))
}

// StepDevice scores every queued slot against the stores as they are now and
// writes the k best per store (1 <= k <= 64) as a parsed batch of capacity =
// SelectCapacity(k) packets: dOutPkts, dSel, dCount, dOutReqs, dOutWords
// (2*capacity slots), dOutSigs (2*capacity*64 bytes), dOutScores. The picks
// and the slots of mark <= 0 leave the pool. Asynchronous on stream.
func (p *Pool) StepDevice(k, capacity int, dOutPkts, dSel, dCount, dOutReqs, dOutWords, dOutSigs, dOutScores,
	stream unsafe.Pointer) error {
	rc := C.hg_stores_pool_step_device(p.h, C.uint32_t(k), C.size_t(capacity), (*C.hg_packet)(dOutPkts),
		(*C.uint32_t)(dSel), (*C.uint32_t)(dCount), (*C.hg_request)(dOutReqs), (*C.uint64_t)(dOutWords),
		(*C.uint8_t)(dOutSigs), (*C.int32_t)(dOutScores), stream)
	if rc != C.HG_OK {
		return p.s.e.fail(rc)
	}
	return nil
}

// Count is the number of slots queued now (synchronous).
func (p *Pool) Count() (int, error) {
	var n C.size_t
	rc := C.hg_stores_pool_count(p.h, &n)
	if rc != C.HG_OK {
		return 0, p.s.e.fail(rc)
	}
	return int(n), nil
}

// Read returns the receiver's queued slots in queue order, at most max of
// them (for tests and diagnosis; synchronous).
func (p *Pool) Read(receiver, max int) ([]PooledSlot, error) {
	if max <= 0 {
		return nil, nil
	}
	pkts := make([]C.hg_packet, max)
	ind := make([]byte, max)
	marks := make([]int32, max)
	var n C.size_t
	rc := C.hg_stores_pool_read(p.h, C.uint32_t(receiver), C.size_t(max), &pkts[0], bytePtr(ind), codePtr(marks), &n)
	if rc != C.HG_OK {
		return nil, p.s.e.fail(rc)
	}
	m := int(n)
	if m > max {
		m = max
	}
	out := make([]PooledSlot, m)
	for i := range out {
		out[i] = PooledSlot{Origin: int(pkts[i].origin), Receiver: int(pkts[i].receiver), Level: int(pkts[i].level),
			Individual: ind[i] != 0, Mark: marks[i]}
	}
	return out, nil
}

// Clear empties the pool.
func (p *Pool) Clear() error {
	rc := C.hg_stores_pool_clear(p.h)
	if rc != C.HG_OK {
		return p.s.e.fail(rc)
	}
	return nil
}

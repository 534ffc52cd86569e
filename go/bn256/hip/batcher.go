package hip

import "sync"

// single is one independent check: a 128-byte key marshal and a 64-byte
// signature marshal.
type single struct {
	pk, sig []byte
}

type job struct {
	msg  []byte
	agg  *Request
	one  *single
	done chan error
}

// batcher merges concurrent PublicKey.VerifySignature calls into launches
// (SURVEY.md §8(b) option 1: no Handel change). One goroutine takes the
// first queued job, drains whatever else is queued (up to maxBatch) and
// submits it (flush): the single checks as one launch whatever their messages,
// the aggregate checks as one C call per message. There
// is no timer: while one launch runs the next batch accumulates, so the batch
// width follows the number of concurrent callers (k Handel instances per
// process, simul/node/main.go:63-131) without adding latency to a lone caller.
type batcher struct {
	e  *Engine
	ch chan *job
	wg sync.WaitGroup
}

const maxBatch = 4096

func (e *Engine) batch() *batcher {
	e.bOnce.Do(func() {
		e.b = &batcher{e: e, ch: make(chan *job, maxBatch)}
		e.b.wg.Add(1)
		go e.b.run()
	})
	return e.b
}

// submit queues one check and waits for its verdict (the error
// PublicKey.VerifySignature returns).
func (e *Engine) submit(msg []byte, agg *Request, one *single) error {
	j := &job{msg: msg, agg: agg, one: one, done: make(chan error, 1)}
	e.batch().ch <- j
	return <-j.done
}

func (b *batcher) run() {
	defer b.wg.Done()
	for {
		j, ok := <-b.ch
		if !ok {
			return
		}
		jobs := []*job{j}
	drain:
		for len(jobs) < maxBatch {
			select {
			case j2, ok := <-b.ch:
				if !ok {
					break drain
				}
				jobs = append(jobs, j2)
			default:
				break drain
			}
		}
		b.flush(jobs)
	}
}

// flush submits one drained set of jobs. Every single-signature job goes into
// ONE VerifyBatchMsgs call, each check on its own message (hashedMessage runs
// per check on the device), so callers on different messages still share a
// launch. Aggregate jobs need the per-message GT tables of the context and stay
// grouped by message, one C call per group.
func (b *batcher) flush(jobs []*job) {
	var ones []*job
	groups := map[string][]*job{}
	var order []string
	for _, j := range jobs {
		if j.agg == nil {
			ones = append(ones, j)
			continue
		}
		k := string(j.msg)
		if _, ok := groups[k]; !ok {
			order = append(order, k)
		}
		groups[k] = append(groups[k], j)
	}
	if len(ones) > 0 {
		msgs := make([][]byte, len(ones))
		pks := make([]byte, 0, 128*len(ones))
		sigs := make([]byte, 0, 64*len(ones))
		for i, j := range ones {
			msgs[i] = j.msg
			pks = append(pks, j.one.pk...)
			sigs = append(sigs, j.one.sig...)
		}
		codes, err := b.e.VerifyBatchMsgs(msgs, pks, sigs)
		b.finish(ones, codes, err)
	}
	for _, k := range order {
		g := groups[k]
		reqs := make([]Request, len(g))
		for i, j := range g {
			reqs[i] = *j.agg
		}
		codes, _, err := b.e.VerifyAggregate([]byte(k), reqs, false)
		b.finish(g, codes, err)
	}
}

func (b *batcher) finish(g []*job, codes []int32, err error) {
	for i, j := range g {
		if err != nil {
			j.done <- err // the whole submission failed: no verdict, not "valid"
		} else {
			j.done <- b.e.CodeError(codes[i])
		}
	}
}

func (b *batcher) close() {
	close(b.ch)
	b.wg.Wait()
}
